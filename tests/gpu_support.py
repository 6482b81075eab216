"""What the GPU tests share: the fence every output buffer stands in, the byte
comparisons, the guarded render of a frame and of a ray list, the collection of
a reflect kernel's own layers, and the bodies of the composition tests (tilings,
schedule, formats).  TEST INFRASTRUCTURE ONLY.

No test file imports another: what two of them need is here, or, when it builds
a scene or a frame, in tests/cases.py.  torch is imported inside functions, so
collection works without a device; the helpers run on CPU tensors against a
stand-in renderer too (tests/test_gpu_support_ref.py) and synchronise only a
GPU.  pytest does not rewrite the assertions of a module that is no test file:
every assertion here says what differed."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

import env_ref as ER
import lights_ref as LR
import reflect_ref as RR
import ssaa_ref
from cases import LIGHTS, SHAPES, fast_case  # noqa: F401 (SHAPES: for the tests)
from fast_paths import ALL
from parity import quantize
from sdf3d_amd import abi, renderer as R

f32 = np.float32
ROOT = Path(__file__).resolve().parent.parent


# ---- the fence --------------------------------------------------------------------------

FILL = 0xA5        # the byte of every guard row, and of a buffer before its call
GUARD = 8          # guard rows behind (and with `front` in front of) a buffer


def fenced(torch, device, shape, dtype, guard=GUARD, front=False):
    """A tensor of `shape` inside an allocation filled with FILL bytes, with
    `guard` rows (of shape[1:]) behind it and, with `front`, as many in front:
    hand it to the call, then ask `untouched` of it.  (Frames and ray lists
    take 8 rows, points 64 on both sides, the flat outputs of the queries 64
    elements or more; a front guard is a multiple of 16 bytes in all of them.)"""
    rows, rest = int(shape[0]), tuple(int(n) for n in shape[1:])
    row = int(np.prod(rest, dtype=np.int64)) * torch.empty((), dtype=dtype).element_size()
    lo = guard if front else 0
    raw = torch.full(((lo + rows + guard) * row,), FILL, dtype=torch.uint8, device=device)
    x = raw.view(dtype).reshape(lo + rows + guard, *rest)[lo:lo + rows]
    x.fence = (raw, lo * row, (lo + rows) * row)
    return x


def untouched(torch, x):
    """Every guard byte around `x` (of `fenced`) is still FILL."""
    raw, lo, hi = x.fence
    return bool((raw[:lo] == FILL).all()) and bool((raw[hi:] == FILL).all())


def _sync(torch, device):
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize()


# ---- comparisons and small helpers ---------------------------------------------------------

def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same(a, b):
    """One shape, one dtype, the same bytes."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def bitwise_eq(a, b):
    """Elementwise: bit for bit, NaN equal to NaN (the queries' outputs)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == "f":
        word = np.uint32 if a.dtype.itemsize == 4 else a.dtype
        return ((np.ascontiguousarray(a).view(word) == np.ascontiguousarray(b).view(word))
                | (np.isnan(a) & np.isnan(b)))
    return a == b


def ndiff(a, b):
    """The number of 32-bit words in which two outputs of one shape differ."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, \
        f"ndiff of {a.dtype}{a.shape} and {b.dtype}{b.shape}"
    return int((a.view(np.uint32) != b.view(np.uint32)).sum())


def rgba_of(rgb):
    out = np.ones(rgb.shape[:2] + (4,), dtype=f32)
    out[..., :3] = rgb
    return out


def read_ppm(path):
    data = Path(path).read_bytes()
    parts = data.split(b"\n", 3)
    assert parts[0] == b"P6", f"{path}: not a P6 file ({parts[0]!r})"
    w, h = map(int, parts[1].split())
    return np.frombuffer(parts[3], dtype=np.uint8).reshape(h, w, 3)


def with_precision(frame, prec):
    f = frame.copy()
    f.params.precision = prec
    return f


def sdf_main(*args, **kw):
    """The C++ host program run with `args`: the completed process."""
    exe = ROOT / "sdf3d_amd" / "bin" / "sdf_main"
    assert exe.exists(), "build() must produce sdf3d_amd/bin/sdf_main"
    return subprocess.run([str(exe), *map(str, args)], capture_output=True, text=True,
                          timeout=120, **kw)


def ptr(x):
    """x's address for the C ABI (None: NULL).  A fenced tensor of no rows still
    has one, in front of its guard, where torch gives an empty view's as 0."""
    if x is None:
        return None
    raw, lo, _ = getattr(x, "fence", (x, 0, 0))
    return C.c_void_p(raw.data_ptr() + lo * (raw is not x))


# ---- guarded renders ------------------------------------------------------------------------

def render(rd, frame, t=None, steps=True, schedule=None, **shading):
    """Renderer.render into fenced buffers: (rgba, steps or None) as NumPy
    arrays, with the rows the call may not touch checked -- the guard rows, and
    under SDF_TILING_FRAME_ROWS the rows the tiling does not own come back as
    they were, FILL bytes.  `shading`: lights, light_flags, materials, reflect,
    env, as Renderer.render takes them."""
    import torch
    p = frame.params
    rows = R.buffer_rows(p.height, t)
    buf = fenced(torch, rd.device, (rows, p.width, R.channels(p.output_format)),
                 R.torch_dtype(p.output_format))
    sbuf = fenced(torch, rd.device, R.steps_shape(frame, t), torch.int32) if steps else None
    rd.render(frame, t, out=buf, steps=sbuf if steps else False, schedule=schedule, **shading)
    _sync(torch, rd.device)
    assert untouched(torch, buf), "colour buffer: rows past the end were written"
    assert not steps or untouched(torch, sbuf), "steps buffer: rows past the end were written"
    return buf.cpu().numpy(), (sbuf.cpu().numpy() if steps else None)


def both(rd, frame, t=None, **shading):
    """The frame rendered without a steps buffer (the instantiation where the
    shortcuts are active) and with one: the colours must agree bit for bit.
    Returns (rgba, steps)."""
    a, _ = render(rd, frame, t, steps=False, **shading)
    b, st = render(rd, frame, t, steps=True, **shading)
    assert same(a, b), f"renders with and without a steps buffer differ in {ndiff(a, b)} words"
    return a, st


def shade_rays(rd, f, O, D, unit, steps=True, **shading):
    """Renderer.render_rays into fenced buffers: (rgba (n, ch), steps (n, 2) or
    None) as NumPy."""
    import torch
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=f32).reshape(-1, 3)).to(rd.device)
    o, d = dev(O), dev(D)
    n = o.shape[0]
    fmt = f.params.output_format
    buf = fenced(torch, rd.device, (n, R.channels(fmt)), R.torch_dtype(fmt))
    sbuf = fenced(torch, rd.device, (n, 2), torch.int32) if steps else None
    rd.render_rays(f, o, d, unit=unit, out=buf, steps=sbuf if steps else False, **shading)
    _sync(torch, rd.device)
    assert untouched(torch, buf), "colour buffer: entries past the end were written"
    assert not steps or untouched(torch, sbuf), "steps buffer: entries past the end were written"
    return buf.cpu().numpy(), (sbuf.cpu().numpy() if steps else None)


def both_rays(rd, f, O, D, unit, **shading):
    a, _ = shade_rays(rd, f, O, D, unit, steps=False, **shading)
    b, st = shade_rays(rd, f, O, D, unit, steps=True, **shading)
    assert same(a, b), f"calls with and without a steps buffer differ in {ndiff(a, b)} words"
    return a, st


def cam_rays(rd, f):
    o, d = rd.camera_rays(f)
    rd.torch.cuda.synchronize()
    return o.cpu().numpy().reshape(-1, 3), d.cpu().numpy().reshape(-1, 3)


def tiles_streams(rd, f, first, second):
    """`f` (SDF_FORMAT_TILES) rendered with the shading `first` and with `second`
    into zeroed buffers (a stream has alignment gaps the encoder does not
    write): one stream.  Returns the two buffers and the stream's length."""
    import torch
    size = R.tiles_bytes(f.params.width, f.params.height)
    a, b = (torch.zeros(size, dtype=torch.uint8, device=rd.device) for _ in range(2))
    rd.render(f, out=a, **first)
    rd.render(f, out=b, **second)
    torch.cuda.synchronize()
    n = R.tiles_stream_bytes(a)
    assert n == R.tiles_stream_bytes(b) and n > abi.TILES_HEADER_BYTES, "the streams' lengths differ"
    assert torch.equal(a[:n], b[:n]), "the streams' bytes differ"
    return a, b, n


def own_layers(call, bounces, strength):
    """The kernel's own layer colours, weights and steps by `layer = j` passes,
    where call(reflect) gives (rgba, steps) of a frame or of a ray list: C, W
    [..., J, 3], steps [..., J, 2], alive [..., J] (a traced layer took a
    primary step)."""
    Cs, Ws, Ss = [], [], []
    for j in range(bounces + 1):
        cj, sj = call(RR.reflect(bounces, strength, j))
        wj, wsj = call(RR.reflect(bounces, strength, j, abi.REFLECT_WEIGHT))
        assert np.array_equal(sj, wsj), f"layer {j}: the colour and the weight pass count differently"
        assert (cj[..., 3] == 1).all() and (wj[..., 3] == 1).all(), f"layer {j}: alpha is not 1"
        Cs.append(cj[..., :3])
        Ws.append(wj[..., :3])
        Ss.append(sj)
    Cj, Wj, Sj = (np.stack(v, axis=-2) for v in (Cs, Ws, Ss))
    alive = Sj[..., 0] > 0
    # a path that has ended leaves zeros
    for a, what in ((Cj, "colour"), (Wj, "weight")):
        assert (bits(a[~alive]) == 0).all(), f"a {what} that is not zero on a layer no path reached"
    assert (Sj[~alive] == 0).all(), "steps counted on a layer no path reached"
    return Cj, Wj, Sj, alive


def rays_fast_deviation(rd, name, bounces, dispatch=None, frame_out=None):
    """env_ref.fast_deviation of cases.fast_case(name, dispatch) shaded from its
    camera rays under SKY | SUN | FOG, the per-layer steps taken by `layer`
    passes.  `frame_out`: a dict that receives the case (f, mats, lights, env,
    o, d) and the fast composite `out`."""
    f, mats = fast_case(name, dispatch)
    lights, env = [LIGHTS[0]], ER.environment(ALL)
    o, d = cam_rays(rd, f)
    kw = dict(lights=lights, materials=mats, env=env)
    _, _, Sj, alive = own_layers(lambda r: both_rays(rd, f, o, d, True, reflect=r, **kw), bounces, 1.0)
    out, st = both_rays(rd, f, o, d, True, reflect=RR.reflect(bounces, 1.0), **kw)
    assert np.array_equal(st, Sj.sum(axis=1)), "the composite's steps are not the layers' sum"
    if frame_out is not None:
        frame_out.update(f=f, mats=mats, lights=lights, env=env, o=o, d=d, out=out)
    W, H, J = f.params.width, f.params.height, bounces + 1
    return ER.fast_deviation(f, mats, lights, env, bounces, out.reshape(H, W, 4),
                             Sj.reshape(H, W, J, 2), alive.reshape(H, W, J))


# ---- single-light pieces of the build's own (lights, materials) --------------------------------

_OWN = {}


def spec_frame(f):
    """`f` with material amb = dif = 0 and ref = 1: its colour is spec exactly
    (fma(spec, 1, fma(dif, 0, 0 * ao)) in fast precision)."""
    g = f.copy()
    for c in range(3):
        g.material.amb[c], g.material.dif[c], g.material.ref[c] = 0.0, 0.0, 1.0
    return g


def own_light(rd, f, light, key=None):
    """(terms, spec, steps) of the build's own single-light renders of `f`
    under `light`: terms from SDF_FORMAT_SHADE32F, spec from the colour of
    spec_frame, the steps of the plain render.  Shared under `key`."""
    if key is not None and key in _OWN:
        return _OWN[key]
    g = LR.with_light(f, light)
    g.params.output_format = abi.FORMAT_SHADE32F
    terms, steps = both(rd, g)
    spec = both(rd, spec_frame(LR.with_light(f, light)))[0][..., 0].copy()
    assert np.isfinite(terms).all() and np.isfinite(spec).all(), "a term or spec is not finite"
    if f.params.precision == abi.PRECISION_EXACT:
        want = LR.spec_exact(terms[..., 2], f.material.shininess)
        assert same(spec, want), f"spec differs from spec_exact in {ndiff(spec, want)} words"
    for a in (terms, spec, steps):
        a.setflags(write=False)
    if key is not None:
        _OWN[key] = (terms, spec, steps)
    return terms, spec, steps


# ---- the composition tests' bodies ----------------------------------------------------------

def hi_frame(f):
    """The S W x S H frame whose pixels are `f`'s sub-samples."""
    s = R.samples(f)
    g = f.copy()
    g.params.width, g.params.height, g.params.samples = s * f.params.width, s * f.params.height, 0
    return g


def hi_tiling(t, s):
    """`t` with block_rows * S: the sub-sample frame's tiling."""
    return abi.sdf_tiling(t.block_rows * s, t.first_block, t.block_stride, t.flags, t.block_run,
                          t.run_step)


def owned_row_index(height, t):
    """Frame rows a tiling owns, ascending (sdf_abi.h sdf_tiling)."""
    run, step = max(t.block_run, 1), max(t.run_step, 1)
    rows = []
    for y in range(height):
        b = y // t.block_rows
        if b < t.first_block:
            continue
        o = (b - t.first_block) % t.block_stride
        if o % step == 0 and o // step < run:
            rows.append(y)
    return np.asarray(rows, dtype=np.int64)


def sub_rows(rows, s):
    return (rows[:, None] * s + np.arange(s)[None, :]).reshape(-1)


def check_tilings(rd, f, world, shares, **shading):
    """Every rank's share of `f` (RGBA32F, S x S supersampled or plain) under
    the tiling of `world` ranks, packed and under SDF_TILING_FRAME_ROWS: the
    rows of the whole frame and its steps, every row seen exactly once; a
    supersampled share is the high-resolution render under the scaled tiling,
    resolved; rows a rank does not own stay FILL.  Returns the whole frame
    and steps."""
    s = R.samples(f)
    w, h = f.params.width, f.params.height
    whole, whole_st = both(rd, f, **shading)
    packed = np.full_like(whole, np.nan)
    packed_st = np.full_like(whole_st, -7)
    seen = np.zeros(h, dtype=int)
    for rank in range(world):
        at = f"rank {rank} of {world}, shares {shares}"
        t = R.tiling(rank, world, 8, shares=shares)
        rows = owned_row_index(h, t)
        srows = sub_rows(rows, s)
        assert len(rows) == R.owned_rows(h, t), f"{at}: owns {R.owned_rows(h, t)} rows, not {len(rows)}"
        seen[rows] += 1
        # packed: the rank's rows, dense
        out, st = both(rd, f, t, **shading)
        assert out.shape == (len(rows), w, 4) and st.shape == (s * len(rows), s * w, 2), \
            f"{at}: packed shapes {out.shape}, {st.shape}"
        assert same(out, whole[rows]), f"{at}: packed rows differ in {ndiff(out, whole[rows])} words"
        assert np.array_equal(st, whole_st[srows]), f"{at}: packed steps differ"
        packed[rows] = out
        packed_st[srows] = st
        if s > 1 and len(rows):
            hi, hi_st = render(rd, hi_frame(f), hi_tiling(t, s), **shading)
            assert same(out, ssaa_ref.resolve(hi, s)) and np.array_equal(st, hi_st), \
                f"{at}: not the high-resolution render under the scaled tiling"
        # frame rows: owned rows at their places, the others untouched
        tf = R.tiling(rank, world, 8, frame_rows=True, shares=shares)
        fr, fr_st = both(rd, f, tf, **shading)
        assert fr.shape == whole.shape and fr_st.shape == whole_st.shape, \
            f"{at}: FRAME_ROWS shapes {fr.shape}, {fr_st.shape}"
        other = np.setdiff1d(np.arange(h), rows)
        assert same(fr[rows], whole[rows]), \
            f"{at}: FRAME_ROWS rows differ in {ndiff(fr[rows], whole[rows])} words"
        assert np.array_equal(fr_st[srows], whole_st[srows]), f"{at}: FRAME_ROWS steps differ"
        assert (bits(fr[other]) == FILL).all(), f"{at}: a colour row it does not own was written"
        assert (bits(fr_st[sub_rows(other, s)]) == FILL).all(), \
            f"{at}: a steps row it does not own was written"
    assert (seen == 1).all(), f"rows not owned exactly once: {np.nonzero(seen != 1)[0]}"
    assert same(packed, whole) and np.array_equal(packed_st, whole_st), \
        "the ranks' packed rows do not make up the frame"
    return whole, whole_st


def check_scheduled(rd, f, after=None, **shading):
    """Three renders of `f` under a schedule of its (sub-sample) rows, each with
    and without a steps buffer, equal the unscheduled render, and the schedule
    served them: order() is a permutation of the 8-row blocks.  `after(sch)`
    runs before the schedule is closed.  Returns the unscheduled (rgba,
    steps)."""
    ref, ref_st = both(rd, f, **shading)
    rows = R.samples(f) * f.params.height
    sch = rd.schedule(rows, period=1)
    try:
        for i in range(3):
            out, st = render(rd, f, steps=True, schedule=sch, **shading)
            assert same(out, ref), f"scheduled render {i} differs in {ndiff(out, ref)} words"
            assert np.array_equal(st, ref_st), f"scheduled render {i}: steps differ"
            out, _ = render(rd, f, steps=False, schedule=sch, **shading)
            assert same(out, ref), f"scheduled render {i} without steps differs in {ndiff(out, ref)} words"
        order = sch.order()
        assert sorted(order) == list(range((rows + 7) // 8)), f"order() is no permutation: {order}"
        if after is not None:
            after(sch)
    finally:
        sch.close()
    return ref, ref_st


def check_formats(rd, f, full, **shading):
    """The 16-bit, 8-bit and three-channel renders of `f` are the conversions
    of `full`, its RGBA32F render."""
    for fmt in (abi.FORMAT_RGBA16F, abi.FORMAT_RGBA8, abi.FORMAT_RGB32F):
        g = f.copy()
        g.params.output_format = fmt
        out, _ = both(rd, g, **shading)
        assert same(out, quantize(full, fmt)), f"format {fmt} is not the converted RGBA32F colour"


# ---- the query and mesh entry points through the C ABI (query, mesh, offsets) -----------------

PAD = 64           # guard rows behind every output of a query, a mesh or a gradient


def dev(rd, a):
    return rd.torch.from_numpy(np.ascontiguousarray(a)).to(rd.device)


def stream_of(rd):
    return C.c_void_p(rd.torch.cuda.current_stream(rd.device).cuda_stream)


def out_buf(rd, n, comps, dtype, want=True):
    """A fenced output of n entries of `comps` components (None unless `want`)."""
    if not want:
        return None
    return fenced(rd.torch, rd.device, (n, comps) if comps > 1 else (n,), dtype, guard=PAD)


def taken(rd, buf):
    """The output as NumPy, after checking that the bytes behind it survived."""
    if buf is None:
        return None
    assert untouched(rd.torch, buf), "the guard behind an output was overwritten"
    return buf.cpu().numpy()


def trace(rd, f, o, d, n=None, t=True, steps=True, normal=True, prim=True):
    """sdf_trace of the first n rays through the C ABI into fenced buffers."""
    torch = rd.torch
    n = len(o) if n is None else n
    O, D = dev(rd, o), dev(rd, d)
    bt = out_buf(rd, n, 1, torch.float32, t)
    bs = out_buf(rd, n, 1, torch.int32, steps)
    bn = out_buf(rd, n, 3, torch.float32, normal)
    bp = out_buf(rd, n, 1, torch.int32, prim)
    h = abi.sdf_hits(ptr(bt), ptr(bs), ptr(bn), ptr(bp))
    rc = rd.lib.sdf_trace(C.byref(f.scene), C.byref(f.params), ptr(O), ptr(D), n, C.byref(h),
                          stream_of(rd))
    abi.check(rc, "sdf_trace")
    torch.cuda.synchronize()
    return {"t": taken(rd, bt), "steps": taken(rd, bs), "normal": taken(rd, bn),
            "prim": taken(rd, bp)}


def sample(rd, f, P, n=None, normal=True):
    """sdf_sample of the first n points through the C ABI into fenced buffers."""
    torch = rd.torch
    n = len(P) if n is None else n
    Pd = dev(rd, P)
    bd = out_buf(rd, n, 1, torch.float32)
    bn = out_buf(rd, n, 3, torch.float32, normal)
    rc = rd.lib.sdf_sample(C.byref(f.scene), C.byref(f.params), ptr(Pd), n, ptr(bd), ptr(bn),
                           stream_of(rd))
    abi.check(rc, "sdf_sample")
    torch.cuda.synchronize()
    return {"dist": taken(rd, bd), "normal": taken(rd, bn)}


def mesh_count(rd, f, g):
    """sdf_mesh_count through the C ABI: (workspace, its size, the four counts)."""
    torch = rd.torch
    nbytes = int(rd.lib.sdf_mesh_workspace_bytes(C.byref(g)))
    assert nbytes > 0, "sdf_mesh_workspace_bytes gave no size"
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=rd.device)
    cn = out_buf(rd, 4, 1, torch.int64)
    rc = rd.lib.sdf_mesh_count(C.byref(f.scene), C.byref(f.params), C.byref(g), ptr(ws), nbytes,
                               ptr(cn), stream_of(rd))
    abi.check(rc, "sdf_mesh_count")
    torch.cuda.synchronize()
    return ws, nbytes, tuple(int(x) for x in taken(rd, cn))


def mesh_emit(rd, f, g, ws, nbytes, cap_v, cap_t, normal=True, prim=True):
    """sdf_mesh_emit into fenced buffers of exactly the capacities given."""
    torch = rd.torch
    bv = out_buf(rd, cap_v, 3, torch.float32)
    bt = out_buf(rd, cap_t, 3, torch.int32)
    bn = out_buf(rd, cap_v, 3, torch.float32, normal)
    bp = out_buf(rd, cap_v, 1, torch.int32, prim)
    out = abi.sdf_mesh_out(ptr(bv), cap_v, ptr(bt), cap_t, ptr(bn), ptr(bp))
    rc = rd.lib.sdf_mesh_emit(C.byref(f.scene), C.byref(f.params), C.byref(g), ptr(ws), nbytes,
                              C.byref(out), stream_of(rd))
    abi.check(rc, "sdf_mesh_emit")
    torch.cuda.synchronize()
    return {"verts": taken(rd, bv), "tris": taken(rd, bt), "normal": taken(rd, bn),
            "prim": taken(rd, bp)}


def raw_mesh(rd, f, spec, dense=False, normal=True, prim=True):
    g = R.grid(*spec, dense=dense)
    ws, nbytes, cn = mesh_count(rd, f, g)
    got = mesh_emit(rd, f, g, ws, nbytes, cn[0], cn[1], normal, prim)
    got["counts"] = cn
    return got


def mesh_mismatches(got, ref):
    bad = {}
    for k in ("verts", "tris", "normal", "prim"):
        a, b = got[k], ref[k]
        bad[k] = -1 if a.shape != b.shape else int((~bitwise_eq(a, b)).sum())
    return bad
