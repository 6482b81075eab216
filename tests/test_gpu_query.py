"""GPU tests of the query entry points (sdf_trace, sdf_trace_camera,
sdf_sample; include/sdf_abi.h "Queries") against tests/query_ref.py, the NumPy
reference over the CPU oracle's point probes: in exact precision bit for bit on
every ray, pixel and point, on every dispatch path; in fast precision within a
measured bound, on every dispatch path too (tests/fast_paths.py: the bound of
the fixed variants on scenes of the same arithmetic, and the fast result not
the exact one's bits).

Sizes: the 200-ray set (three full waves and a tail of 8) plus five hand-made
rays; frames of 64 x 36 and 37 x 23 (ragged tiles); a 17 x 13 x 11 point grid.
Every output buffer is followed by 64 sentinel elements, which must survive.
A scene's GPU results and its reference are computed once and shared."""
import ctypes as C

import numpy as np
import pytest

import fast_paths as FP
import materials_ref as MR
import query_ref as Q
from cases import JIT_SEEDS
from cases import query_frame as frame_of
from fast_paths import FAST_BOUND_N, FAST_BOUND_T
from gpu_support import bitwise_eq, dev, ndiff, out_buf, ptr, sample, sdf_main, taken, trace
from sdf3d_amd import abi, scenes

pytestmark = pytest.mark.gpu

f32 = np.float32
EXACT, FAST = abi.PRECISION_EXACT, abi.PRECISION_FAST
# REF, C1 and C4 are the built-in variants 1, 2 and 3; J<seed>: cases.JIT_SEEDS,
# run-time specialised under SDF_DISPATCH_AUTO
KINDS = ["REF", "C1", "C4", "C4-generic", "C4-unculled", "J0", "J4", "J6", "C5"]
def all_rays():
    o, d = Q.ray_set()
    ho, hd = Q.hand_rays()
    return np.concatenate([o, ho]), np.concatenate([d, hd])


ZERO = Q.N_RAYS + Q.ZERO_DIR     # the zero direction's index in all_rays()


_cache = {}


def exact_run(rd, kind):
    """(GPU results, reference, run-time compilations of the first call and of
    a second) of the 205 rays on `kind` in exact precision, computed once."""
    if kind not in _cache:
        f = frame_of(kind)
        o, d = all_rays()
        n0 = rd.lib.sdf_jit_count()
        got = trace(rd, f, o, d)
        n1 = rd.lib.sdf_jit_count()
        again = trace(rd, f, o, d)
        n2 = rd.lib.sdf_jit_count()
        for k in got:
            assert np.all(bitwise_eq(got[k], again[k])), f"{kind}: {k} differs between two calls"
        _cache[kind] = (got, Q.trace(f, o, d), n1 - n0, n2 - n1)
    return _cache[kind]


def report(kind, got, ref, rays):
    bad = {k: int((~bitwise_eq(got[k], ref[k]))[rays].sum()) for k in ("t", "steps", "normal", "prim")}
    print(f"{kind}: {len(rays)} rays, {int(ref['hit'][rays].sum())} hit; mismatches {bad}")
    return bad


# 1. exact precision, buffer rays ------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_exact_rays_equal_the_reference(renderer, kind):
    """t (NaN equals NaN), steps, normal and prim of the 200-ray set and the
    four hand-made rays of finite direction equal the reference on every ray,
    bit for bit; a custom signature compiles exactly once."""
    got, ref, jit_first, jit_second = exact_run(renderer, kind)
    rays = np.array([i for i in range(len(ref["t"])) if i != ZERO])
    bad = report(kind, got, ref, rays)
    assert bad == {"t": 0, "steps": 0, "normal": 0, "prim": 0}
    assert jit_first == (1 if kind in JIT_SEEDS else 0) and jit_second == 0


@pytest.mark.parametrize("kind", KINDS)
def test_exact_zero_direction_equals_the_reference(renderer, kind):
    """The hand-made ray with a zero direction (D = NaN): t, steps, normal and
    prim equal the reference's, NaN equal to NaN -- +INF after one step where the
    scene's selects drop the NaN (REF, C1), NaN after max_steps where a smooth
    operator keeps it.  The kernels march such a ray with the scene spec's
    selects (render_kernel.inc sel_query), not with the evaluators built for
    the validated range."""
    got, ref, _, _ = exact_run(renderer, kind)
    z = np.array([ZERO])
    print(f"{kind}: zero direction: kernel t {got['t'][ZERO]} steps {got['steps'][ZERO]} prim "
          f"{got['prim'][ZERO]} normal {got['normal'][ZERO]}; reference t {ref['t'][ZERO]} steps "
          f"{ref['steps'][ZERO]} prim {ref['prim'][ZERO]} normal {ref['normal'][ZERO]}")
    bad = report(kind, got, ref, z)
    assert bad == {"t": 0, "steps": 0, "normal": 0, "prim": 0}


@pytest.mark.parametrize("kind", KINDS)
def test_exact_nonfinite_directions_equal_the_reference(renderer, kind):
    """Directions of infinite or NaN length (query_ref.odd_rays: D with NaN
    components beside zero ones), alone and mixed into a wave of ordinary
    rays, whose results they must not change."""
    f = frame_of(kind)
    oo, od = Q.odd_rays()
    got, ref = trace(renderer, f, oo, od), Q.trace(f, oo, od)
    bad = report(kind, got, ref, np.arange(len(oo)))
    assert bad == {"t": 0, "steps": 0, "normal": 0, "prim": 0}
    full, _, _, _ = exact_run(renderer, kind)
    o, d = all_rays()
    o, d = o[:64].copy(), d[:64].copy()
    at = [3, 17, 40, 63]
    o[at], d[at] = oo[:4], od[:4]
    mixed = trace(renderer, f, o, d)
    rest = np.array([i for i in range(64) if i not in at])
    for k in mixed:
        assert np.all(bitwise_eq(mixed[k][rest], full[k][rest])), k
        assert np.all(bitwise_eq(mixed[k][at], got[k][:4])), k


# 2. independence of n and lane ----------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_results_do_not_depend_on_n(renderer, n):
    """The first n results equal those of the 205-ray run, bit for bit, and the
    guard behind each output is untouched (gpu_support.taken)."""
    full, _, _, _ = exact_run(renderer, "C4")
    o, d = all_rays()
    got = trace(renderer, frame_of("C4"), o, d, n=n)
    for k in got:
        assert len(got[k]) == n and np.all(bitwise_eq(got[k], full[k][:n])), k


def test_no_rays_write_nothing(renderer):
    o, d = all_rays()
    got = trace(renderer, frame_of("C4"), o, d, n=0)      # every element is guard
    assert all(len(v) == 0 for v in got.values())
    empty = renderer.torch.zeros((0, 3), dtype=renderer.torch.float32, device=renderer.device)
    h = renderer.trace(frame_of("C4"), empty, empty)
    assert h.t.shape == (0,) and h.normal.shape == (0, 3)
    dist, nrm = renderer.sample(frame_of("C4"), empty, normal=True)
    assert dist.shape == (0,) and nrm.shape == (0, 3)


# 3. output selection ---------------------------------------------------------------
@pytest.mark.parametrize("sel", [("t",), ("prim",), ("normal",), ("t", "normal"),
                                 ("steps", "prim")])
def test_output_selection_does_not_change_the_bits(renderer, sel):
    """Only t, only prim, normal without steps, ...: the same bits as with all
    four outputs."""
    full, _, _, _ = exact_run(renderer, "C4")
    o, d = all_rays()
    got = trace(renderer, frame_of("C4"), o, d, **{k: k in sel for k in full})
    for k in full:
        if k in sel:
            assert np.all(bitwise_eq(got[k], full[k])), k
        else:
            assert got[k] is None


def test_renderer_trace_is_the_abi_call(renderer):
    """Renderer.trace returns the C call's values as torch tensors."""
    full, _, _, _ = exact_run(renderer, "C4")
    o, d = all_rays()
    h = renderer.trace(frame_of("C4"), dev(renderer, o), dev(renderer, d))
    renderer.torch.cuda.synchronize()
    for k in full:
        assert np.all(bitwise_eq(getattr(h, k).cpu().numpy(), full[k])), k
    h = renderer.trace(frame_of("C4"), dev(renderer, o), dev(renderer, d), normal=False,
                       prim=False)
    assert h.normal is None and h.prim is None and h.t.shape == (len(o),)


# 4. camera rays ----------------------------------------------------------------------
def render_steps(rd, f):
    _, st = rd.render(f, steps=True)
    rd.torch.cuda.synchronize()
    return st.cpu().numpy()[..., 0]


@pytest.mark.parametrize("wh", [(64, 36), (37, 23)])
@pytest.mark.parametrize("name", ["REF", "C4", "C5"])
def test_camera_rays(renderer, name, wh):
    """steps equal sdf_render's primary counts in both precisions, with
    SHADOW | AO and with flags 0; in exact precision t, normal and prim equal
    the reference on every pixel."""
    check_camera_rays(renderer, name, wh)


@pytest.mark.parametrize("name", ["C4-generic", "C4-unculled", "J4"])
def test_camera_rays_dispatch_paths(renderer, name):
    """The same on the launch paths test_camera_rays does not take: the generic
    kernel culled and unculled, and a run-time specialised scene.  40 x 17
    pixels: five tiles and a ragged column across, a ragged last 8-row block."""
    check_camera_rays(renderer, name, (40, 17))


def check_camera_rays(renderer, name, wh):
    W, H = wh
    for prec in (EXACT, FAST):
        f = frame_of(name, prec, wh)
        h = renderer.trace_camera(f)
        renderer.torch.cuda.synchronize()
        got = {k: getattr(h, k).cpu().numpy() for k in ("t", "steps", "normal", "prim")}
        assert got["t"].shape == (H, W) and got["normal"].shape == (H, W, 3)
        for flags in (abi.FLAG_SHADOW | abi.FLAG_AO, 0):
            g = f.copy()
            g.params.flags = flags
            rs = render_steps(renderer, g)
            print(f"{name} {wh} precision {prec} flags {flags}: "
                  f"{int((rs != got['steps']).sum())} step counts differ from the render's")
            assert np.array_equal(rs, got["steps"])
        if prec == EXACT:
            O, D = Q.camera_rays(f)
            ref = Q.hits(f, O, D)
            bad = {k: int((~bitwise_eq(got[k].reshape(ref[k].shape), ref[k])).sum())
                   for k in ("t", "steps", "normal", "prim")}
            print(f"{name} {wh}: {int(ref['hit'].sum())} of {W * H} pixels hit; mismatches {bad}")
            assert bad == {"t": 0, "steps": 0, "normal": 0, "prim": 0}


def test_camera_rays_unsupported(renderer):
    f = frame_of("C4")
    f.params.samples = 2
    with pytest.raises(abi.SdfError) as e:
        renderer.trace_camera(f)
    assert e.value.code == abi.SDF_E_UNSUPPORTED


# 5. points -----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_points_equal_the_oracle(renderer, kind):
    """dist and normal on the 17 x 13 x 11 grid equal oracle.scene_sdf and
    oracle.normal, bit for bit, in exact precision."""
    torch = renderer.torch
    f = frame_of(kind)
    P = Q.grid()
    n = len(P)
    bd = out_buf(renderer, n, 1, torch.float32)
    bn = out_buf(renderer, n, 3, torch.float32)
    Pd = dev(renderer, P)
    rc = renderer.lib.sdf_sample(C.byref(f.scene), C.byref(f.params), ptr(Pd), n, ptr(bd),
                                 ptr(bn), None)
    abi.check(rc, "sdf_sample")
    torch.cuda.synchronize()
    dist, nrm = taken(renderer, bd), taken(renderer, bn)
    rdist, rnrm = Q.scene_sdf(f, P), Q.normals(f, P)
    assert (rdist < 0).sum() >= 5 and (P[:, 1] < 0).sum() >= 100    # inside, and below the floor
    bad = (int((~bitwise_eq(dist, rdist)).sum()), int((~bitwise_eq(nrm, rnrm)).sum()))
    print(f"{kind}: {n} points, {int((rdist < 0).sum())} inside; mismatches dist, normal {bad}")
    assert bad == (0, 0)
    d2, n2 = renderer.sample(f, dev(renderer, P), normal=True)
    d1, none = renderer.sample(f, dev(renderer, P))
    torch.cuda.synchronize()
    assert none is None and np.all(bitwise_eq(d2.cpu().numpy(), dist))
    assert np.all(bitwise_eq(d1.cpu().numpy(), dist)) and np.all(bitwise_eq(n2.cpu().numpy(), nrm))


# 6. fast precision, buffer rays --------------------------------------------------------
def counted(rd, key, call):
    """call()'s result, twice: on a run-time specialised path (`key` names the
    family's fast kernel on it, else None) the first call compiles exactly one
    kernel the first time the key is used in this process, the second none;
    the two results are the same bits."""
    count = rd.lib.sdf_jit_count
    n0 = count()
    got = call()
    n1 = count()
    again = call()
    n2 = count()
    if key is not None:
        assert (n1 - n0, n2 - n1) == (FP.first_use(key), 0), (key, n1 - n0, n2 - n1)
    for k in got:
        assert np.all(bitwise_eq(got[k], again[k])), f"{key}: {k} differs between two calls"
    return got


@pytest.mark.parametrize("name", ["REF", "C4", "C5", "C4-generic", "C4-unculled", "C4-carved"])
def test_fast_rays_within_the_measured_bound(renderer, name):
    """Fast precision on the 200-ray set against the reference
    (query_ref.fast_deviation): t against the replay at the kernel's own step
    counts on every ray, normal on the rays whose steps agree with the
    oracle's, prim on every hit ray whose closest owner decision is at least
    materials_ref.GAP wide (at most 2 % are not: test_query_ref.py,
    test_fast_paths_ref.py).  The generic kernel culled and unculled and the
    run-time specialised C4-carved are held to the bound measured on the fixed
    variants: C4's primitives and smooth kernel, the same scene in exact
    precision as reference.  And the fast unit ran: some word differs from the
    exact result of the same call, which equals the oracle's."""
    f = frame_of(name, FAST)
    o, d = Q.ray_set()
    got = counted(renderer, ("trace", name) if name in FP.JIT else None,
                  lambda: trace(renderer, f, o, d))
    r = Q.fast_deviation(frame_of(name), o, d, got, MR.GAP)
    exact = exact_run(renderer, name)[0]
    differ = {k: ndiff(got[k], exact[k][:len(o)]) for k in ("t", "normal")}
    print(f"{name}: fast deviation {r}; bounds t {FAST_BOUND_T:.3e} normal {FAST_BOUND_N:.3e}; "
          f"words differing from the exact result {differ}")
    assert r["prim_left_out"] <= 0.02 * r["hit"]
    assert r["prim_wrong"] == 0
    assert r["t"] <= FAST_BOUND_T
    assert r["normal"] <= FAST_BOUND_N
    assert differ["t"] + differ["normal"] > 0, "the exact kernel's bits: the fast unit did not run"


# 6b. fast precision, points ------------------------------------------------------------
@pytest.mark.parametrize("kind", ["REF", "C4", "C4-generic", "C4-unculled", "C4-carved", "C5"])
def test_fast_points_within_the_bound(renderer, kind):
    """Fast sdf_sample on the 17 x 13 x 11 grid, on all five launch paths,
    against the oracle (fast_paths.point_deviation).  dist is held to
    FAST_BOUND_T, which bounds a whole march's t -- a sum of up to max_steps of
    these evaluations -- in the same relative metric over REF, C4 and C5; one
    evaluation is held to no looser bound.  normal is held to FAST_BOUND_N,
    which bounds the same tap code at hit points, there with P itself
    deviating; at most 2 % of the points, where the oracle's own readings
    disagree, are left out.  Some word differs from the exact result of the
    same call (test_points_equal_the_oracle holds that one); C4-carved
    compiles one kernel, once.  On the generic path the first n results do not
    depend on n."""
    f, P = frame_of(kind, FAST), Q.grid()
    got = counted(renderer, ("sample", kind) if kind in FP.JIT else None,
                  lambda: sample(renderer, f, P))
    exact = sample(renderer, frame_of(kind), P)
    differ = {k: ndiff(got[k], exact[k]) for k in got}
    r = FP.point_deviation(frame_of(kind), P, got["dist"], got["normal"])
    print(f"{kind}: fast deviation {r}; bounds dist {FAST_BOUND_T:.3e} normal {FAST_BOUND_N:.3e}; "
          f"words differing from the exact result {differ}")
    assert r["normal_left_out"] <= FP.LEFT_OUT_SHARE * r["points"]
    assert r["dist"] <= FAST_BOUND_T
    assert r["normal"] <= FAST_BOUND_N
    assert differ["dist"] + differ["normal"] > 0, "the exact kernel's bits: the fast unit did not run"
    if kind == "C4-generic":
        for n in (1, 63, 64, 65):
            part = sample(renderer, f, P, n=n)
            for k in part:
                assert len(part[k]) == n and np.all(bitwise_eq(part[k], got[k][:n])), (k, n)
        only = sample(renderer, f, P, normal=False)
        assert only["normal"] is None and np.all(bitwise_eq(only["dist"], got["dist"]))


# 7. the C++ host program -----------------------------------------------------------------
def test_cpp_host_program_pick(renderer, tmp_path):
    """sdf_main --pick X,Y prints the record Renderer.trace_camera gives for
    that pixel (the last frame's camera; frame 1 of 2 is yaw 180)."""
    f = scenes.config("C3", 160, 90)                                  # sdf_main's csg8
    scenes.set_view(f, scenes.orbit_view(180.0, 0.0))
    h = renderer.trace_camera(f)
    renderer.torch.cuda.synchronize()
    prim = h.prim.cpu().numpy()
    # a pixel on the sphere-side blend and one of the sky
    ys, xs = np.nonzero(prim > 0)
    picks = [(int(xs[len(xs) // 2]), int(ys[len(ys) // 2]))]
    ys, xs = np.nonzero(prim < 0)
    picks.append((int(xs[0]), int(ys[0])))
    for x, y in picks:
        r = sdf_main("--pick", f"{x},{y}", "160", "90", "2", tmp_path / "f.ppm", "csg8")
        assert r.returncode == 0, r.stderr
        line = [l for l in r.stdout.splitlines() if l.startswith(f"pick {x},{y}: ")]
        assert len(line) == 1, r.stdout
        v = line[0].split(": ")[1].split()
        assert len(v) == 6
        assert np.all(bitwise_eq(f32(v[0]), h.t[y, x].cpu().numpy()))
        assert int(v[1]) == int(h.steps[y, x]) and int(v[2]) == int(prim[y, x])
        assert np.all(bitwise_eq(np.array(v[3:], dtype=f32), h.normal[y, x].cpu().numpy()))
