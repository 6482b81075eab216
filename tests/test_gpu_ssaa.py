"""GPU tests of fused supersampling (sdf_params.samples = 2, 4; include/sdf_abi.h
"Supersampling"): a supersampled W x H frame is the S W x S H frame resolved
in the contract's tree order (tests/ssaa_ref.py), bit for bit and on every
pixel -- against the CPU oracle in exact precision, against the build's own
high-resolution render in both precisions -- for every output format, tiling,
dispatch path and a schedule, with the sub-samples' step counts.

Shapes: 37 x 23 output for S = 2 (74 x 46 sub-samples: partial 8 x 8 tiles in
x and y, a last block of 7 output rows) and 21 x 10 for S = 4 (84 x 40).  Every
render here writes into buffers followed by 8 sentinel rows, which must
survive (`render`)."""
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import oracle
import ssaa_ref
from parity import quantize
from sdf3d_amd import abi, renderer as R, scenes

pytestmark = pytest.mark.gpu

SHAPES = {2: (37, 23), 4: (21, 10)}
FRAMES = [("REF", 0), ("C2", 1), ("C3", 2), ("C4", 0), ("C5", 3), ("C1", 0)]
PRECS = [abi.PRECISION_EXACT, abi.PRECISION_FAST]
GUARD = 8          # sentinel rows after every buffer
FILL = 0xA5        # their bytes


def lo_frame(cfg, pose, s, prec=abi.PRECISION_EXACT, wh=None):
    w, h = wh or SHAPES[s]
    f = scenes.config(cfg, w, h, precision=prec, pose=pose)
    f.params.samples = s
    return f


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


_ORACLE = {}


def oracle_hi(cfg, pose, s):
    """The oracle's S W x S H frame and steps of (cfg, pose) at the test
    shape: rendered once, shared, read-only, asserted finite."""
    key = (cfg, pose, s)
    if key not in _ORACLE:
        rgba, steps = oracle.render(hi_frame(lo_frame(cfg, pose, s)))
        rgba.setflags(write=False)
        steps.setflags(write=False)
        _ORACLE[key] = (rgba, steps)
    rgba, steps = _ORACLE[key]
    assert np.isfinite(rgba).all(), key
    return rgba, steps


def _guarded(torch, device, shape, dtype):
    rows = shape[0]
    n = (rows + GUARD) * int(np.prod(shape[1:])) * torch.empty((), dtype=dtype).element_size()
    raw = torch.full((n,), FILL, dtype=torch.uint8, device=device)
    return raw.view(dtype).reshape(rows + GUARD, *shape[1:])


def _sentinel(torch, x):
    return bool((x.contiguous().view(-1).view(torch.uint8) == FILL).all())


def render(rd, frame, t=None, steps=True, schedule=None):
    """renderer.render into sentinel-filled buffers with GUARD rows behind
    them: returns (rgba, steps or None) as NumPy arrays WITH the rows the
    call may not touch checked -- the guard rows, and under
    SDF_TILING_FRAME_ROWS the rows the tiling does not own (returned as they
    are, sentinel bytes)."""
    import torch
    p = frame.params
    rows = R.buffer_rows(p.height, t)
    shape = (rows, p.width, R.channels(p.output_format))
    buf = _guarded(torch, rd.device, shape, R.torch_dtype(p.output_format))
    sshape = R.steps_shape(frame, t)
    sbuf = _guarded(torch, rd.device, sshape, torch.int32) if steps else None
    rd.render(frame, t, out=buf[:rows], steps=sbuf[:sshape[0]] if steps else False,
              schedule=schedule)
    torch.cuda.synchronize()
    assert _sentinel(torch, buf[rows:]), "colour buffer: rows past the end were written"
    if steps:
        assert _sentinel(torch, sbuf[sshape[0]:]), "steps buffer: rows past the end were written"
    return buf[:rows].cpu().numpy(), (sbuf[:sshape[0]].cpu().numpy() if steps else None)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def both(rd, frame, t=None):
    """The frame rendered without a steps buffer (the instantiation where the
    exact shadow skip is active) and with one: the colours must agree bit for
    bit.  Returns (rgba, steps)."""
    a, _ = render(rd, frame, t, steps=False)
    b, st = render(rd, frame, t, steps=True)
    assert same(a, b), "renders with and without a steps buffer differ"
    return a, st


# ---- 1. exact precision against the oracle -----------------------------------

@pytest.mark.parametrize("s", [2, 4])
@pytest.mark.parametrize("cfg,pose", FRAMES)
def test_exact_equals_resolved_oracle(renderer, cfg, pose, s):
    ref, ref_steps = oracle_hi(cfg, pose, s)
    want = ssaa_ref.resolve(ref, s)
    out, st = both(renderer, lo_frame(cfg, pose, s))
    assert st.shape == ref_steps.shape and np.array_equal(st, ref_steps)
    assert same(out, want), int((out.view(np.uint32) != want.view(np.uint32)).sum())


# ---- 2. both precisions against the build's own high-resolution render -------

def check_against_own_render(rd, f, steps=True):
    s = R.samples(f)
    hi, hi_st = render(rd, hi_frame(f), steps=steps)
    assert np.isfinite(hi).all()
    out, st = render(rd, f, steps=steps)
    want = ssaa_ref.resolve(hi, s)
    assert same(out, want), int((out.view(np.uint32) != want.view(np.uint32)).sum())
    if steps:
        assert np.array_equal(st, hi_st)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("s", [2, 4])
@pytest.mark.parametrize("cfg,pose", FRAMES)
def test_equals_own_render_resolved(renderer, cfg, pose, s, prec):
    oracle_hi(cfg, pose, s)                    # the frame is finite
    f = lo_frame(cfg, pose, s, prec)
    check_against_own_render(renderer, f, steps=False)
    check_against_own_render(renderer, f, steps=True)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("s", [2, 4])
@pytest.mark.parametrize("dispatch", [abi.DISPATCH_GENERIC, abi.DISPATCH_UNCULLED])
def test_generic_kernel_paths(renderer, dispatch, s, prec):
    oracle_hi("C3", 2, s)
    f = lo_frame("C3", 2, s, prec)
    f.params.dispatch = dispatch
    check_against_own_render(renderer, f, steps=False)
    check_against_own_render(renderer, f, steps=True)


def unmatched_scene(s, prec):
    """plane, box, torus in hard union: no built-in variant, so
    SDF_DISPATCH_AUTO compiles its kernel at run time (hipRTC)."""
    f = lo_frame("C3", 2, s, prec)
    f.scene.count = 3
    scenes._prim(f.scene, 1, abi.PRIM_BOX, abi.OP_UNION, 0.0, -0.4, 0.15, 0.0, 0.15, 0.15, 0.15)
    scenes._prim(f.scene, 2, abi.PRIM_TORUS, abi.OP_UNION, 0.0, 0.4, 0.1, 0.0, 0.2, 0.06)
    return f


@pytest.mark.parametrize("prec", PRECS)
def test_runtime_specialised_scene(renderer, prec):
    before = renderer.lib.sdf_jit_count()
    for s in (2, 4):                           # one kernel serves both (S is a uniform)
        f = unmatched_scene(s, prec)
        ref, _ = oracle.render(hi_frame(f))
        assert np.isfinite(ref).all()
        check_against_own_render(renderer, f, steps=False)
        if s == 2:
            check_against_own_render(renderer, f, steps=True)
        if prec == abi.PRECISION_EXACT:
            out, _ = render(renderer, f, steps=False)
            assert same(out, ssaa_ref.resolve(ref, s))
    if os.environ.get("SDF3D_JIT") != "0":
        # the plain and the supersampling kernel, with and without steps
        assert renderer.lib.sdf_jit_count() - before == 4


# ---- 3. samples 0 and 1 ------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
def test_one_sample_is_the_plain_render(renderer, prec):
    f = lo_frame("C3", 2, 0, prec, wh=SHAPES[2])
    ref, _ = oracle.render(f)
    assert np.isfinite(ref).all()
    base, base_st = both(renderer, f)
    if prec == abi.PRECISION_EXACT:
        assert same(base, ref)
    f.params.samples = 1
    one, one_st = both(renderer, f)
    assert same(one, base) and np.array_equal(one_st, base_st)
    assert one_st.shape == (23, 37, 2)


# ---- 4. output formats ---------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("s", [2, 4])
def test_formats_convert_the_resolved_colour(renderer, s, prec):
    oracle_hi("C3", 2, s)
    f = lo_frame("C3", 2, s, prec)
    full, _ = render(renderer, f, steps=False)
    for fmt in (abi.FORMAT_RGBA16F, abi.FORMAT_RGBA8, abi.FORMAT_RGB32F):
        g = f.copy()
        g.params.output_format = fmt
        out, _ = both(renderer, g)
        assert same(out, quantize(full, fmt)), fmt


# ---- 5. tilings ------------------------------------------------------------------

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


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("s", [2, 4])
@pytest.mark.parametrize("world,shares", [(3, (1, 1)), (2, (1, 2))])
def test_tilings(renderer, world, shares, s, prec):
    oracle_hi("C3", 2, s)
    f = lo_frame("C3", 2, s, prec)
    w, h = f.params.width, f.params.height
    whole, whole_st = both(renderer, f)
    packed = np.full_like(whole, np.nan)
    packed_st = np.full_like(whole_st, -7)
    seen = np.zeros(h, dtype=int)
    for rank in range(world):
        t = R.tiling(rank, world, 8, shares=shares)
        rows = owned_row_index(h, t)
        assert len(rows) == R.owned_rows(h, t)
        seen[rows] += 1
        # packed: the rank's rows, dense; they deinterleave into the frame
        out, st = both(renderer, f, t)
        assert out.shape == (len(rows), w, 4) and st.shape == (s * len(rows), s * w, 2)
        packed[rows] = out
        packed_st[sub_rows(rows, s)] = st
        # ... and equal the high-resolution render under the scaled tiling
        if len(rows):
            hi, hi_st = render(renderer, hi_frame(f), hi_tiling(t, s))
            assert same(out, ssaa_ref.resolve(hi, s)) and np.array_equal(st, hi_st)
        # frame rows: owned rows at their places, the others untouched
        tf = R.tiling(rank, world, 8, frame_rows=True, shares=shares)
        fr, fr_st = both(renderer, f, tf)
        assert fr.shape == whole.shape and fr_st.shape == whole_st.shape
        other = np.setdiff1d(np.arange(h), rows)
        assert same(fr[rows], whole[rows])
        assert np.array_equal(fr_st[sub_rows(rows, s)], whole_st[sub_rows(rows, s)])
        assert (bits(fr[other]) == FILL).all() and (bits(fr_st[sub_rows(other, s)]) == FILL).all()
    assert (seen == 1).all()
    assert same(packed, whole) and np.array_equal(packed_st, whole_st)


# ---- 6. bounds ---------------------------------------------------------------------

@pytest.mark.parametrize("s", [2, 4])
@pytest.mark.parametrize("fmt", [abi.FORMAT_RGBA32F, abi.FORMAT_RGBA8, abi.FORMAT_RGB32F])
def test_nothing_is_written_past_the_buffers(renderer, s, fmt):
    """`render` holds every call of this file to it; here once on its own, for
    the widest and the narrowest pixel and a tiling whose last block is cut."""
    oracle_hi("C4", 0, s)
    f = lo_frame("C4", 0, s, abi.PRECISION_FAST)
    f.params.output_format = fmt
    for t in (None, R.tiling(1, 2, 8), R.tiling(0, 2, 8, frame_rows=True)):
        out, st = render(renderer, f, t, steps=True)
        rows = R.buffer_rows(f.params.height, t)
        assert out.shape[0] == rows and st.shape[0] == s * rows


# ---- 7. schedule -------------------------------------------------------------------

@pytest.mark.parametrize("s,prec", [(2, abi.PRECISION_EXACT), (4, abi.PRECISION_FAST)])
def test_scheduled_supersampled_render(renderer, s, prec):
    oracle_hi("C3", 2, s)
    f = lo_frame("C3", 2, s, prec)
    ref, ref_st = render(renderer, f, steps=True)
    rows = s * f.params.height                 # the schedule's rows are sub-sample rows
    sch = renderer.schedule(rows, period=1)
    try:
        for _ in range(3):
            out, st = render(renderer, f, steps=True, schedule=sch)
            assert same(out, ref) and np.array_equal(st, ref_st)
        nb = (rows + 7) // 8
        assert sorted(sch.order()) == list(range(nb))    # it did serve these renders
        # a schedule for the output rows does not fit: launch order, same frame
        other = renderer.schedule(f.params.height, period=1)
        try:
            for _ in range(2):
                out, _ = render(renderer, f, steps=False, schedule=other)
                assert same(out, ref)
            assert other.order() == []
        finally:
            other.close()
    finally:
        sch.close()


# ---- 8. the C++ host program ---------------------------------------------------------

def read_ppm(path):
    data = Path(path).read_bytes()
    parts = data.split(b"\n", 3)
    assert parts[0] == b"P6"
    w, h = map(int, parts[1].split())
    return np.frombuffer(parts[3], dtype=np.uint8).reshape(h, w, 3)


def test_cpp_host_program_samples_argument(renderer, tmp_path):
    exe = Path(__file__).resolve().parent.parent / "sdf3d_amd" / "bin" / "sdf_main"
    assert exe.exists(), "build() must produce sdf3d_amd/bin/sdf_main"
    f = scenes.config("C3", 160, 90, precision=abi.PRECISION_EXACT)   # sdf_main's default
    scenes.set_view(f, scenes.orbit_view(180.0, 0.0))                 # frame 1 of 2: yaw 180
    f.params.samples = 2
    ref, _ = oracle.render(hi_frame(f))
    assert np.isfinite(ref).all()
    f.params.output_format = abi.FORMAT_RGBA8
    want, _ = render(renderer, f, steps=False)
    assert same(want, quantize(ssaa_ref.resolve(ref, 2), abi.FORMAT_RGBA8))
    out = tmp_path / "f.ppm"
    r = subprocess.run([str(exe), "160", "90", "2", str(out), "csg8", "2"], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    img = read_ppm(out)
    assert img.shape == (90, 160, 3)
    assert np.array_equal(img, want[::-1, :, :3])
