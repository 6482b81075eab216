"""GPU tests of caller-supplied rays (sdf_render_rays, sdf_camera_rays;
include/sdf_abi.h "Rays"): sdf_camera_rays against tests/query_ref.py bit for
bit; in exact precision the camera's rays shaded with SDF_RAYS_UNIT against the
frame renders, colours and steps bit for bit, on every dispatch path and format;
rays that are no camera's -- the reflected rays of the CPU reference's walk --
against that reference; the kernel's normalisation; inactive rays; the ray
count; the run-time compiled kernel; fast precision within the environment
tests' measured bound; the host program's --projection.

The ray set is a 37 x 23 frame's: 851 rays, 13 full waves and 19 lanes.  Every
call writes into buffers followed by sentinel rows, which must survive, and
every case is shaded with and without a steps buffer, which must not change the
colours."""
import ctypes as C
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import env_ref as ER
import fast_paths as FP
import query_ref as QR
import reflect_ref as RR
from cases import LIGHTS, fast_case, mats_of, the_frame, walk_of
from cases import rays_jit_case as jit_case
from fast_paths import ALL, WEIGHT
from fast_paths import ENV_BOUND as FAST_BOUND
from gpu_support import (FILL, bits, cam_rays, fenced, ndiff, rays_fast_deviation, read_ppm, same,
                         sdf_main, untouched)
from gpu_support import both as frame_both
from gpu_support import both_rays as both
from gpu_support import shade_rays as shade
from parity import quantize
from sdf3d_amd import abi, scenes

pytestmark = pytest.mark.gpu

f32 = np.float32
EXACT, FAST = abi.PRECISION_EXACT, abi.PRECISION_FAST
SKY, SUN, FOG = abi.ENV_SKY, abi.ENV_SUN, abi.ENV_FOG
W, H = ER.SHAPE
N = W * H
ROOT = Path(__file__).resolve().parent.parent


def test_the_shape():
    assert (W, H) == (37, 23) and N == 851 == 13 * 64 + 19


# ---- helpers ---------------------------------------------------------------------------

def shading(f, n, flags, reflect, eflags):
    """The keyword arguments Renderer.render and Renderer.render_rays share."""
    return dict(lights=LIGHTS[:n], light_flags=flags, materials=mats_of(f), reflect=reflect,
                env=None if eflags is None else ER.environment(eflags))


# ---- 1. camera rays ------------------------------------------------------------------------

def aspect_frame(prec=EXACT):
    f = the_frame("C3", 2, prec)
    f.camera.aspect = 1.25
    return f


@pytest.mark.parametrize("make", [lambda p: the_frame("REF", 0, p), lambda p: the_frame("C3", 2, p),
                                  aspect_frame], ids=["REF-p0", "C3-p2", "aspect"])
def test_camera_rays_are_the_renders(renderer, make):
    o, d = cam_rays(renderer, make(EXACT))
    wo, wd = QR.camera_rays(make(EXACT))
    assert o.shape == d.shape == (N, 3)
    assert same(o, wo) and same(d, wd), (ndiff(o, wo), ndiff(d, wd))
    for prec in (EXACT, FAST):
        _, d = cam_rays(renderer, make(prec))
        length = np.sqrt((d.astype(np.float64) ** 2).sum(axis=1))
        print(f"precision {prec}: |D| - 1 in [{length.min() - 1:.3e}, {length.max() - 1:.3e}]")
        assert length.max() <= 1 + 2.0 ** -22          # what SDF_RAYS_UNIT needs


def test_camera_rays_null_output_and_samples(renderer):
    import torch
    f = the_frame("C3", 2)
    o, d = cam_rays(renderer, f)
    lib = renderer.lib
    for which in (0, 1):
        buf = fenced(torch, renderer.device, (N, 3), torch.float32)
        ptr = C.c_void_p(buf.data_ptr())
        rc = lib.sdf_camera_rays(C.byref(f.camera), C.byref(f.params), None if which else ptr,
                                 ptr if which else None, None)
        torch.cuda.synchronize()
        assert rc == abi.SDF_OK
        assert same(buf.cpu().numpy(), d if which else o) and untouched(torch, buf)
    g = f.copy()
    g.params.samples = 2
    with pytest.raises(abi.SdfError) as e:
        renderer.camera_rays(g)
    assert e.value.code == abi.SDF_E_UNSUPPORTED


# ---- 2. parity with the frame renders ------------------------------------------------------

# (frame, pose, dispatch, lights, light flags, bounces, layer, reflect flags, env flags, format)
A, G, U = abi.DISPATCH_AUTO, abi.DISPATCH_GENERIC, abi.DISPATCH_UNCULLED
CLR = abi.LIGHTS_COLOR
F32, F16, U8, RGB = (abi.FORMAT_RGBA32F, abi.FORMAT_RGBA16F, abi.FORMAT_RGBA8, abi.FORMAT_RGB32F)
PARITY = [
    ("REF", 0, A, 1, 0, 0, -1, 0, None, F32), ("REF", 0, A, 3, CLR, 2, -1, 0, ALL, RGB),
    ("C4", 0, A, 3, CLR, 2, -1, 0, ALL, F32), ("C4", 0, A, 1, 0, 0, -1, 0, ALL, F32),
    ("C4", 0, A, 1, 0, 2, -1, 0, None, F16), ("C4", 0, A, 3, CLR, 2, 1, 0, ALL, F32),
    ("C4", 0, A, 1, 0, 2, 1, WEIGHT, None, F32), ("C5", 0, A, 1, 0, 2, -1, 0, ALL, F32),
    ("C5", 0, A, 3, CLR, 0, -1, 0, None, F32), ("EJ", 2, A, 3, CLR, 2, -1, 0, ALL, F32),
    ("EJ", 2, A, 1, 0, 2, -1, 0, None, F32), ("C3", 2, G, 1, 0, 2, -1, 0, None, U8),
    ("C3", 2, U, 3, CLR, 0, -1, 0, ALL, F32), ("C3", 2, U, 3, CLR, 2, -1, 0, None, F32),
]


@pytest.mark.parametrize("name,pose,dispatch,n,flags,bounces,layer,rflags,eflags,fmt", PARITY)
def test_camera_rays_shade_to_the_frame(renderer, name, pose, dispatch, n, flags, bounces, layer,
                                        rflags, eflags, fmt):
    """render_rays(camera_rays, unit=True) is Renderer.render flattened, colours
    and steps bit for bit (exact precision)."""
    f = the_frame(name, pose, EXACT, dispatch)
    f.params.output_format = fmt
    kw = shading(f, n, flags, RR.reflect(bounces, 1.0, layer, rflags), eflags)
    want, want_st = frame_both(renderer, f, **kw)
    o, d = cam_rays(renderer, f)
    out, st = both(renderer, f, o, d, True, **kw)
    want = want.reshape(N, -1)
    print(f"differing words {int((bits(out) != bits(want)).sum())} of {bits(out).size}")
    assert same(out, want)
    assert np.array_equal(st, want_st.reshape(N, 2))
    if bounces == 0 and eflags is None:
        # reflect NULL is bounces 0 with layer -1, env NULL none
        kw["reflect"] = None
        out2, st2 = both(renderer, f, o, d, True, **kw)
        assert same(out2, out) and np.array_equal(st2, st)


# ---- 3. rays that are not camera rays -------------------------------------------------------

OWN_FRAMES = [("REF", 0), ("C3", 2), ("C4", 0), ("C5", 0)]
_OWN = {}


def own_rays(name, pose):
    """The reflected rays of the CPU reference's walk (2 bounces, strength 1, one
    light) as a ray set of their own: (O, D, active, walk sliced to layers 1..)."""
    if (name, pose) not in _OWN:
        f = the_frame(name, pose)
        w = walk_of(name, pose, 2, 1, 0)
        active = w["alive"][:, :, 1].reshape(N)
        ws = {k: (v[:, :, 1:] if isinstance(v, np.ndarray) else v) for k, v in w.items()}
        ws["bounces"] = 1
        # the conditions under which the sliced walk is the ray set's own path:
        # enough rays, and a path goes on past its first layer exactly where the
        # walk's does (the weights restart at W = 1, the walk's carry W_1)
        assert active.mean() >= 0.30, active.mean()
        with np.errstate(invalid="ignore"):
            hit = ~(w["d"][:, :, 1] > f32(f.params.max_dist))
        k1zero = ((f32(1.0) * w["ref"][:, :, 1]).astype(f32) == 0).all(axis=-1)
        goes_on = w["alive"][:, :, 1] & hit & ~k1zero
        assert np.array_equal(goes_on, w["alive"][:, :, 2]), int((goes_on != w["alive"][:, :, 2]).sum())
        _OWN[(name, pose)] = (w["O"][:, :, 1].reshape(N, 3), w["D"][:, :, 1].reshape(N, 3), active, ws)
    return _OWN[(name, pose)]


@pytest.mark.parametrize("eflags", [0, ALL])
@pytest.mark.parametrize("name,pose", OWN_FRAMES)
def test_own_rays_equal_the_reference(renderer, name, pose, eflags):
    """Two calls (the simpler form: normalize need not leave a unit D's bits
    alone).  The active rays, compacted, with unit=True against the reference:
    ER.apply on the walk sliced to layers 1.., which recomputes the weights
    from W = 1, then RR.composite.  Then the whole set with unit=False and a
    zero direction for every pixel whose path did not reach layer 1: those
    entries are all-zero, and the others are the first call's wherever
    normalize leaves D as it is."""
    f = the_frame(name, pose)
    O, D, active, ws = own_rays(name, pose)
    env = ER.environment(eflags)
    e = ER.apply(f, ws, env)
    want = RR.composite(e["C"], e["W"], e["alive"]).reshape(N, 4)
    want_st = e["steps"].sum(axis=2).astype(np.int32).reshape(N, 2)
    assert np.isfinite(want).all()
    kw = dict(lights=LIGHTS[:1], materials=mats_of(f), reflect=RR.reflect(1, 1.0), env=env)
    out, st = both(renderer, f, O[active], D[active], True, **kw)
    print(f"{int(active.sum())} of {N} rays active; differing words {ndiff(out, want[active])}")
    assert same(out, want[active]) and np.array_equal(st, want_st[active])
    out2, st2 = both(renderer, f, O, np.where(active[:, None], D, f32(0.0)), False, **kw)
    assert (bits(out2[~active]) == 0).all() and (st2[~active] == 0).all()
    kept = active & (bits(QR.normalize(D)) == bits(D)).reshape(N, -1).all(axis=1)
    print(f"normalize leaves {int(kept.sum())} of {int(active.sum())} active directions as they are")
    assert kept.any()
    assert same(out2[kept], want[kept]) and np.array_equal(st2[kept], want_st[kept])
    assert (out2[active][:, 3] == 1).all()


# ---- 4. normalisation ------------------------------------------------------------------------

def test_the_kernel_normalises(renderer):
    """Directions scaled by factors in [0.1, 10] with unit=False give the bits of
    unit=True on query_ref.normalize of them (exact precision)."""
    f = the_frame("C4", 0)
    O, D, active, _ = own_rays("C4", 0)
    rng = np.random.default_rng(11)
    scaled = (D[active] * rng.uniform(0.1, 10.0, int(active.sum()))[:, None].astype(f32)).astype(f32)
    kw = shading(f, 3, CLR, RR.reflect(2, 1.0), ALL)
    out, st = both(renderer, f, O[active], scaled, False, **kw)
    want, want_st = both(renderer, f, O[active], QR.normalize(scaled), True, **kw)
    assert same(out, want) and np.array_equal(st, want_st)
    assert np.abs(out[:, :3]).max() > 0.1


# ---- 5. inactive rays ------------------------------------------------------------------------

ODD_AT = [3, 64, 127, 200, 333, 500, 849, 850]    # first, last and inner lanes of several waves


@pytest.mark.parametrize("unit", [False, True])
def test_inactive_rays(renderer, unit):
    """query_ref.odd_rays' directions among the camera's rays: all-zero output
    and steps (0, 0) in every format, and the other rays of their waves keep
    the bits of a call without them.  A ray is inactive when its D has a
    component that is not finite: without SDF_RAYS_UNIT every odd direction
    (normalize gives NaN), with it all but the zero direction, which is finite
    as given -- that ray is marched, and left out of both comparisons."""
    f = the_frame("C4", 0)
    o, d = cam_rays(renderer, f)
    _, odd = QR.odd_rays()
    assert len(odd) == len(ODD_AT)
    d2 = d.copy()
    d2[ODD_AT] = odd
    idx = np.array(ODD_AT)
    inactive = idx if not unit else idx[~np.isfinite(odd).all(axis=1)]
    assert len(inactive) == (8 if not unit else 7)
    rest = np.setdiff1d(np.arange(N), idx)
    for fmt in (F32, F16, U8, RGB):
        g = f.copy()
        g.params.output_format = fmt
        kw = shading(g, 3, CLR, RR.reflect(2, 1.0), ALL)
        clean, clean_st = both(renderer, g, o, d, unit, **kw)
        out, st = both(renderer, g, o, d2, unit, **kw)
        assert (bits(out[inactive]) == 0).all() and (st[inactive] == 0).all(), fmt
        assert same(out[rest], clean[rest]) and np.array_equal(st[rest], clean_st[rest]), fmt
        assert (clean_st[:, 0] > 0).all()
        # without an environment, and with no bounce asked for
        kw = shading(g, 1, 0, None, None)
        out, st = both(renderer, g, o, d2, unit, **kw)
        assert (bits(out[inactive]) == 0).all() and (st[inactive] == 0).all(), fmt


# ---- 6. the ray count ------------------------------------------------------------------------

def test_the_first_n_results_do_not_depend_on_n(renderer):
    import torch
    f = the_frame("C4", 0)
    o, d = cam_rays(renderer, f)
    kw = shading(f, 3, CLR, RR.reflect(2, 1.0), ALL)
    full, full_st = both(renderer, f, o, d, True, **kw)
    for n in (1, 63, 64, 65):
        out, st = both(renderer, f, o[:n], d[:n], True, **kw)
        assert same(out, full[:n]) and np.array_equal(st, full_st[:n]), n
    # n = 0 touches nothing (shade checks the whole of both buffers: all guard)
    out, st = both(renderer, f, o[:0], d[:0], True, **kw)
    assert out.shape == (0, 4) and st.shape == (0, 2)
    rays = abi.sdf_rays(None, None, 0, 0, 0)
    marr = (abi.sdf_material * 8)(*kw["materials"])
    larr = (abi.sdf_light * 3)(*kw["lights"])
    buf = fenced(torch, renderer.device, (4, 4), torch.float32)
    rc = renderer.lib.sdf_render_rays(C.byref(f.scene), larr, 3, CLR, marr, 8, None, None,
                                      C.byref(f.params), C.byref(rays),
                                      C.c_void_p(buf.data_ptr()), C.c_void_p(buf.data_ptr()), None)
    torch.cuda.synchronize()
    assert rc == abi.SDF_OK and untouched(torch, buf) and (bits(buf.cpu().numpy()) == FILL).all()


# ---- 7. the run-time compiled kernel ---------------------------------------------------------

CHILD = """
import sys
import numpy as np
sys.path[:0] = [{root!r}, {tests!r}]
import torch
import cases
import gpu_support as G
from sdf3d_amd import Renderer
rd = Renderer("cuda:0")
f, kw = cases.rays_jit_case()
o, d = G.cam_rays(rd, f)
out, st = G.both_rays(rd, f, o, d, True, **kw)
assert rd.lib.sdf_jit_count() == 0
np.save({out!r}, out)
np.save({st!r}, st)
"""


def test_runtime_specialised_scene_compiles_one_kernel(renderer, tmp_path):
    f, kw = jit_case()
    jit = os.environ.get("SDF3D_JIT") != "0"
    count = renderer.lib.sdf_jit_count
    o, d = cam_rays(renderer, f)
    want, want_st = frame_both(renderer, f, **kw)          # compiles the scene's render kernels
    before = count()
    out, _ = shade(renderer, f, o, d, True, steps=False, **kw)
    assert count() - before == (1 if jit else 0)           # one rays kernel on first use
    for r, ef in ((RR.reflect(0, 1.0), SKY), (RR.reflect(3, 0.5, 2), FOG), (RR.reflect(2, 0.75), ALL)):
        again, _ = shade(renderer, f, o, d, True, steps=False, **dict(kw, reflect=r,
                                                                       env=ER.environment(ef)))
        assert count() - before == (1 if jit else 0)       # none on the second
    assert same(out, again) and same(out, want.reshape(N, 4))
    # step recording and no environment are instantiations of their own
    out2, st = shade(renderer, f, o, d, True, steps=True, **kw)
    assert same(out2, out) and np.array_equal(st, want_st.reshape(N, 2))
    shade(renderer, f, o, d, True, steps=False, **dict(kw, env=None))
    assert count() - before == (3 if jit else 0)
    # the generic kernel in a child process gives the same bits
    paths = dict(root=str(ROOT), tests=str(ROOT / "tests"), out=str(tmp_path / "out.npy"),
                 st=str(tmp_path / "st.npy"))
    r = subprocess.run([sys.executable, "-c", CHILD.format(**paths)], capture_output=True,
                       text=True, timeout=300, env=dict(os.environ, SDF3D_JIT="0"))
    assert r.returncode == 0, r.stderr[-2000:]
    assert same(np.load(paths["out"]), out) and np.array_equal(np.load(paths["st"]), st)


# ---- 8. fast precision -----------------------------------------------------------------------

# case -> (cases.fast_case's frame, dispatch): the fixed variants the bound
# was measured on, then C4 on the generic kernel culled and unculled, the
# run-time specialised EJ (round box, plane, torus under smooth union: kinds and
# an operator of C4's) and the Mandelbulb's unit
FAST_CASES = {"C4": ("C4", None), "C3": ("C3", None), "REF": ("REF", None),
              "C4-generic": ("C4", G), "C4-unculled": ("C4", U), "EJ": ("EJ", None),
              "C5": ("C5", None)}


@pytest.mark.parametrize("bounces", [1, 2])
@pytest.mark.parametrize("case", list(FAST_CASES))
def test_fast_is_near_the_reference(renderer, case, bounces):
    """The fast composite of the camera's rays with SKY | SUN | FOG against the
    reference replayed at the kernel's own per-layer step counts, taken by
    `layer` passes: within fast_paths.ENV_BOUND, the project's measured bound
    for this arithmetic on these rays, with at most ER.BOUNDARY_SHARE of the
    frame left out -- on the fixed variants it was measured on, and with the
    same constant on the generic kernel culled and unculled, a run-time
    specialised scene and the Mandelbulb's unit.  And the fast unit ran: some
    word of the composite differs from the exact result of the same call
    (test_camera_rays_shade_to_the_frame holds that one); the run-time
    specialised scene compiles one rays kernel per instantiation, once."""
    name, dispatch = FAST_CASES[case]
    jit = case == "EJ"
    if jit:     # the two instantiations the case uses: without and with step counts
        f, mats = fast_case(name, dispatch)
        o, d = cam_rays(renderer, f)
        kw = dict(lights=[LIGHTS[0]], materials=mats, reflect=RR.reflect(bounces, 1.0),
                  env=ER.environment(ALL))
        count = renderer.lib.sdf_jit_count
        for steps in (False, True):
            n0 = count()
            shade(renderer, f, o, d, True, steps=steps, **kw)
            n1 = count()
            shade(renderer, f, o, d, True, steps=steps, **kw)
            assert (n1 - n0, count() - n1) == (FP.first_use(("rays", case, steps)), 0), steps
    before = renderer.lib.sdf_jit_count()
    run = {}
    dev, left_out, pixels = rays_fast_deviation(renderer, name, bounces, dispatch, run)
    assert renderer.lib.sdf_jit_count() == before
    g = run["f"].copy()
    g.params.precision = EXACT
    exact, _ = both(renderer, g, run["o"], run["d"], True, lights=run["lights"],
                    materials=run["mats"], reflect=RR.reflect(bounces, 1.0), env=run["env"])
    differ = ndiff(run["out"], exact)
    print(f"{case} bounces {bounces}: largest deviation {dev:.3e}, {left_out} of {pixels} rays "
          f"left out; bound {FAST_BOUND:.3e}; {differ} words differ from the exact result")
    assert left_out <= ER.BOUNDARY_SHARE * pixels
    assert dev <= FAST_BOUND
    assert differ > 0, "the exact kernel's bits: the fast unit did not run"


# ---- 9. the C++ host program -----------------------------------------------------------------

def test_cpp_host_program_projection_option(renderer, tmp_path):
    tail = ["--sky", "--fog", "1,4", "--reflect", "2", str(W), str(H), "2"]
    plain, pin, pano = (tmp_path / n for n in ("plain.ppm", "pinhole.ppm", "equirect.ppm"))
    for out, opt in ((plain, []), (pin, ["--projection", "pinhole"])):
        r = sdf_main(*opt, *tail, out, "csg8")
        assert r.returncode == 0, r.stderr
    assert read_ppm(plain).shape == (H, W, 3)
    assert plain.read_bytes() == pin.read_bytes()
    assert len(np.unique(read_ppm(plain).reshape(-1, 3), axis=0)) > 50
    # a panorama under the sky without its sun: the top row looks at the zenith
    r = sdf_main("--projection", "equirect", "--sky", "--no-sun", W, H, "2", pano, "csg8")
    assert r.returncode == 0, r.stderr
    img = read_ppm(pano)
    assert img.shape == (H, W, 3)
    zenith = quantize(np.array([[[*scenes.SKY_ZENITH, 1.0]]], dtype=f32), U8)[0, 0, :3].astype(int)
    assert np.abs(img[0].astype(int) - zenith).max() <= 1, (img[0], zenith)
    assert r.stdout.count("frame ") == 2
