"""GPU tests of the run-time scene specialiser (sdf3d_amd/csrc/jit.cpp).

A primitive scene whose (kind, op) sequence matches no built-in variant is
rendered, under SDF_DISPATCH_AUTO, by a FixedScene kernel compiled with hipRTC
for that sequence.  It must equal the unculled generic kernel bit for bit in
exact precision (step counts included) and within the parity policy in fast
precision, exactly as the built-in variants do (test_gpu_parity.py
test_specialised_matches_generic, test_culling_exact_on_random_scenes).
"""
import os

import numpy as np
import pytest

from cases import custom_scene
from parity import assert_parity, compare
from sdf3d_amd import abi, scenes

pytestmark = pytest.mark.gpu


def gpu(rd, frame, steps=True):
    import torch
    rgba, st = rd.render(frame, steps=steps)
    torch.cuda.synchronize()
    return rgba.cpu().numpy(), (st.cpu().numpy() if st is not None else None)


def jit_count(rd):
    return rd.lib.sdf_jit_count()


@pytest.mark.parametrize("seed", range(8))
def test_jit_kernel_matches_unculled(renderer, seed):
    rng = np.random.default_rng(100 + seed)
    f = custom_scene(rng, 2 + seed % 7)
    before = jit_count(renderer)
    for prec in (abi.PRECISION_EXACT, abi.PRECISION_FAST):
        f.params.precision = prec
        a, sa = gpu(renderer, f)
        u = f.copy()
        u.params.dispatch = abi.DISPATCH_UNCULLED
        b, sb = gpu(renderer, u)
        if prec == abi.PRECISION_EXACT:
            assert np.array_equal(sa, sb)
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        else:
            assert_parity(compare(f, a, sa, b, sb, ref_is_oracle=False), what=f"jit seed {seed}")
    # a new signature compiles once per precision; the second frame reuses it
    assert jit_count(renderer) - before in (0, 1, 2)
    n = jit_count(renderer)
    gpu(renderer, f)
    assert jit_count(renderer) == n


def test_jit_used_for_unmatched_signature_only(renderer):
    """Built-in variants stay built-in; a reordered CSG8 list is compiled."""
    f = scenes.config("C3", 96, 64)
    n0 = jit_count(renderer)
    gpu(renderer, f)                         # built-in variant 3
    assert jit_count(renderer) == n0
    g = f.copy()
    g.scene.prims[1], g.scene.prims[2] = g.scene.prims[2], g.scene.prims[1]
    a, sa = gpu(renderer, g)
    assert jit_count(renderer) == n0 + 1
    u = g.copy()
    u.params.dispatch = abi.DISPATCH_UNCULLED
    u.params.precision = g.params.precision = abi.PRECISION_EXACT
    a, sa = gpu(renderer, g)
    b, sb = gpu(renderer, u)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.array_equal(sa, sb)


def test_jit_disabled_falls_back_to_generic(renderer):
    rng = np.random.default_rng(7)
    f = custom_scene(rng, 3)
    f.scene.prims[1].kind = abi.PRIM_CYLINDER      # a signature of its own
    f.scene.prims[2].kind = abi.PRIM_CYLINDER
    f.params.precision = abi.PRECISION_EXACT
    os.environ["SDF3D_JIT"] = "0"
    try:
        n0 = jit_count(renderer)
        a, sa = gpu(renderer, f)
        assert jit_count(renderer) == n0
    finally:
        del os.environ["SDF3D_JIT"]
    b, sb = gpu(renderer, f)                   # now specialised
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.array_equal(sa, sb)


def test_jit_tiles_output(renderer):
    """The specialised kernel's TILES instantiation round-trips losslessly."""
    import torch
    rng = np.random.default_rng(11)
    f = custom_scene(rng, 4, 120, 72)
    ref, _ = gpu(renderer, f, steps=False)
    t = f.copy()
    t.params.output_format = abi.FORMAT_TILES
    st, _ = renderer.render(t)
    out = renderer.tiles_decode(st, 1, st.numel(), 120, 72)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), ref.view(np.uint32))
