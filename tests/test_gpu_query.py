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
from sdf3d_amd import abi, scenes
from test_gpu_jit import custom_scene

pytestmark = pytest.mark.gpu

f32 = np.float32
EXACT, FAST = abi.PRECISION_EXACT, abi.PRECISION_FAST
PAD, FILL_F, FILL_I = 64, -777.25, -777
# REF, C1 and C4 are the built-in variants 1, 2 and 3; J<seed>: test_gpu_jit.py's
# custom_scene(100 + seed), signatures with CSG operators that no built-in
# variant has (run-time specialised under SDF_DISPATCH_AUTO)
KINDS = ["REF", "C1", "C4", "C4-generic", "C4-unculled", "J0", "J4", "J6", "C5"]
JIT_SEEDS = {"J0": 0, "J4": 4, "J6": 6}
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


def frame_of(kind, prec=EXACT, wh=(64, 36)):
    if kind in JIT_SEEDS:
        seed = JIT_SEEDS[kind]
        f = custom_scene(np.random.default_rng(100 + seed), 2 + seed % 7, *wh)
    elif kind == "C4-carved":       # run-time specialised, with C4's arithmetic (fast_paths.py)
        f = FP.PATHS[kind](prec, wh)
    else:
        f = scenes.config(kind.split("-")[0], *wh)
        if kind.endswith("-generic"):
            f.params.dispatch = abi.DISPATCH_GENERIC
        if kind.endswith("-unculled"):
            f.params.dispatch = abi.DISPATCH_UNCULLED
    f.params.precision = prec
    return f


def all_rays():
    o, d = Q.ray_set()
    ho, hd = Q.hand_rays()
    return np.concatenate([o, ho]), np.concatenate([d, hd])


ZERO = Q.N_RAYS + Q.ZERO_DIR     # the zero direction's index in all_rays()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else a.dtype)


def same(a, b):
    """Bit for bit, NaN equal to NaN."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == "f":
        return (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))
    return a == b


def dev(rd, a):
    return rd.torch.from_numpy(np.ascontiguousarray(a)).to(rd.device)


def guarded(rd, n, comps, dtype, want=True):
    """n * comps elements followed by PAD sentinels, all set to the sentinel."""
    torch = rd.torch
    if not want:
        return None
    fill = FILL_F if dtype == torch.float32 else FILL_I
    return torch.full((n * comps + PAD,), fill, dtype=dtype, device=rd.device)


def unguard(buf, n, comps):
    """The first n entries, after checking that the sentinels behind them survived."""
    if buf is None:
        return None
    a = buf.cpu().numpy()
    fill = FILL_F if a.dtype == np.float32 else FILL_I
    assert np.all(a[n * comps:] == fill), "sentinels behind an output were overwritten"
    a = a[:n * comps]
    return a.reshape(n, comps) if comps > 1 else a


def ptr(x):
    return C.c_void_p(x.data_ptr()) if x is not None else None


def trace(rd, f, o, d, n=None, t=True, steps=True, normal=True, prim=True):
    """sdf_trace of the first n rays through the C ABI into guarded buffers."""
    torch = rd.torch
    n = len(o) if n is None else n
    O, D = dev(rd, o), dev(rd, d)
    bt = guarded(rd, n, 1, torch.float32, t)
    bs = guarded(rd, n, 1, torch.int32, steps)
    bn = guarded(rd, n, 3, torch.float32, normal)
    bp = guarded(rd, n, 1, torch.int32, prim)
    h = abi.sdf_hits(ptr(bt), ptr(bs), ptr(bn), ptr(bp))
    rc = rd.lib.sdf_trace(C.byref(f.scene), C.byref(f.params), ptr(O), ptr(D), n, C.byref(h),
                          C.c_void_p(torch.cuda.current_stream(rd.device).cuda_stream))
    abi.check(rc, "sdf_trace")
    torch.cuda.synchronize()
    return {"t": unguard(bt, n, 1), "steps": unguard(bs, n, 1), "normal": unguard(bn, n, 3),
            "prim": unguard(bp, n, 1)}


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
            assert np.all(same(got[k], again[k])), f"{kind}: {k} differs between two calls"
        _cache[kind] = (got, Q.trace(f, o, d), n1 - n0, n2 - n1)
    return _cache[kind]


def report(kind, got, ref, rays):
    bad = {k: int((~same(got[k], ref[k]))[rays].sum()) for k in ("t", "steps", "normal", "prim")}
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
        assert np.all(same(mixed[k][rest], full[k][rest])), k
        assert np.all(same(mixed[k][at], got[k][:4])), k


# 2. independence of n and lane ----------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_results_do_not_depend_on_n(renderer, n):
    """The first n results equal those of the 205-ray run, bit for bit, and the
    64 sentinels behind each output are untouched (unguard)."""
    full, _, _, _ = exact_run(renderer, "C4")
    o, d = all_rays()
    got = trace(renderer, frame_of("C4"), o, d, n=n)
    for k in got:
        assert len(got[k]) == n and np.all(same(got[k], full[k][:n])), k


def test_no_rays_write_nothing(renderer):
    o, d = all_rays()
    got = trace(renderer, frame_of("C4"), o, d, n=0)      # unguard checks every element
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
            assert np.all(same(got[k], full[k])), k
        else:
            assert got[k] is None


def test_renderer_trace_is_the_abi_call(renderer):
    """Renderer.trace returns the C call's values as torch tensors."""
    full, _, _, _ = exact_run(renderer, "C4")
    o, d = all_rays()
    h = renderer.trace(frame_of("C4"), dev(renderer, o), dev(renderer, d))
    renderer.torch.cuda.synchronize()
    for k in full:
        assert np.all(same(getattr(h, k).cpu().numpy(), full[k])), k
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
            bad = {k: int((~same(got[k].reshape(ref[k].shape), ref[k])).sum())
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
    bd = guarded(renderer, n, 1, torch.float32)
    bn = guarded(renderer, n, 3, torch.float32)
    Pd = dev(renderer, P)
    rc = renderer.lib.sdf_sample(C.byref(f.scene), C.byref(f.params), ptr(Pd), n, ptr(bd),
                                 ptr(bn), None)
    abi.check(rc, "sdf_sample")
    torch.cuda.synchronize()
    dist, nrm = unguard(bd, n, 1), unguard(bn, n, 3)
    rdist, rnrm = Q.scene_sdf(f, P), Q.normals(f, P)
    assert (rdist < 0).sum() >= 5 and (P[:, 1] < 0).sum() >= 100    # inside, and below the floor
    bad = (int((~same(dist, rdist)).sum()), int((~same(nrm, rnrm)).sum()))
    print(f"{kind}: {n} points, {int((rdist < 0).sum())} inside; mismatches dist, normal {bad}")
    assert bad == (0, 0)
    d2, n2 = renderer.sample(f, dev(renderer, P), normal=True)
    d1, none = renderer.sample(f, dev(renderer, P))
    torch.cuda.synchronize()
    assert none is None and np.all(same(d2.cpu().numpy(), dist))
    assert np.all(same(d1.cpu().numpy(), dist)) and np.all(same(n2.cpu().numpy(), nrm))


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
        assert np.all(same(got[k], again[k])), f"{key}: {k} differs between two calls"
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
    differ = {k: FP.bits_differ(got[k], exact[k][:len(o)]) for k in ("t", "normal")}
    print(f"{name}: fast deviation {r}; bounds t {FAST_BOUND_T:.3e} normal {FAST_BOUND_N:.3e}; "
          f"words differing from the exact result {differ}")
    assert r["prim_left_out"] <= 0.02 * r["hit"]
    assert r["prim_wrong"] == 0
    assert r["t"] <= FAST_BOUND_T
    assert r["normal"] <= FAST_BOUND_N
    assert differ["t"] + differ["normal"] > 0, "the exact kernel's bits: the fast unit did not run"


# 6b. fast precision, points ------------------------------------------------------------
def sample(rd, f, P, n=None, normal=True):
    """sdf_sample of the first n points through the C ABI into guarded buffers."""
    torch = rd.torch
    n = len(P) if n is None else n
    Pd = dev(rd, P)
    bd = guarded(rd, n, 1, torch.float32)
    bn = guarded(rd, n, 3, torch.float32, normal)
    rc = rd.lib.sdf_sample(C.byref(f.scene), C.byref(f.params), ptr(Pd), n, ptr(bd), ptr(bn),
                           C.c_void_p(torch.cuda.current_stream(rd.device).cuda_stream))
    abi.check(rc, "sdf_sample")
    torch.cuda.synchronize()
    return {"dist": unguard(bd, n, 1), "normal": unguard(bn, n, 3)}


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
    differ = {k: FP.bits_differ(got[k], exact[k]) for k in got}
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
                assert len(part[k]) == n and np.all(same(part[k], got[k][:n])), (k, n)
        only = sample(renderer, f, P, normal=False)
        assert only["normal"] is None and np.all(same(only["dist"], got["dist"]))


# 7. the C++ host program -----------------------------------------------------------------
def test_cpp_host_program_pick(renderer, tmp_path):
    """sdf_main --pick X,Y prints the record Renderer.trace_camera gives for
    that pixel (the last frame's camera; frame 1 of 2 is yaw 180)."""
    import subprocess
    from pathlib import Path
    exe = Path(__file__).resolve().parent.parent / "sdf3d_amd" / "bin" / "sdf_main"
    assert exe.exists(), "build() must produce sdf3d_amd/bin/sdf_main"
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
        r = subprocess.run([str(exe), "--pick", f"{x},{y}", "160", "90", "2",
                            str(tmp_path / "f.ppm"), "csg8"], capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 0, r.stderr
        line = [l for l in r.stdout.splitlines() if l.startswith(f"pick {x},{y}: ")]
        assert len(line) == 1, r.stdout
        v = line[0].split(": ")[1].split()
        assert len(v) == 6
        assert np.all(same(f32(v[0]), h.t[y, x].cpu().numpy()))
        assert int(v[1]) == int(h.steps[y, x]) and int(v[2]) == int(prim[y, x])
        assert np.all(same(np.array(v[3:], dtype=f32), h.normal[y, x].cpu().numpy()))
