"""CPU checks of what the GPU tests share (tests/gpu_support.py, tests/cases.py):
the fence sees a write on either side of a buffer and none inside it; the shared
render helpers and composition checks pass on a stand-in renderer that copies
rows of a fixed frame, and each raises when the stand-in makes the mistake the
helper is there to catch; and the scenes whose run-time compilations the GPU
tests count have (kind, op) sequences of their own."""
import numpy as np
import pytest
import torch

import cases
import fast_paths as FP
import gpu_support as G
from sdf3d_amd import abi, renderer as R, scenes

W, H = 37, 23


# ---- 1. the fence ---------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(5,), (5, 3), (3, 37, 4)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.int32, torch.uint8])
@pytest.mark.parametrize("front", [False, True])
def test_fence_sees_the_elements_next_to_the_buffer(dtype, shape, front):
    def element(x, at):
        """The element `at` places from x's first, in or out of x."""
        return x.as_strided((1,), (1,), x.storage_offset() + at)

    x = G.fenced(torch, "cpu", shape, dtype, guard=2, front=front)
    assert tuple(x.shape) == shape and x.dtype == dtype and x.is_contiguous()
    assert G.untouched(torch, x)
    assert (G.bits(x.numpy()) == G.FILL).all()
    x.zero_()                                     # every element inside
    assert G.untouched(torch, x)
    element(x, x.numel())[0] = 0                  # the element just behind
    assert not G.untouched(torch, x)
    if front:
        y = G.fenced(torch, "cpu", shape, dtype, guard=2, front=True)
        element(y, -1)[0] = 0                     # the element just before
        assert not G.untouched(torch, y)


def test_fence_guards_are_as_wide_as_asked():
    x = G.fenced(torch, "cpu", (4, 3), torch.float32, guard=64, front=True)
    raw, lo, hi = x.fence
    assert lo == 64 * 12 and raw.numel() - hi == 64 * 12 and hi - lo == 4 * 12
    x = G.fenced(torch, "cpu", (0, 2), torch.int32)
    assert x.shape == (0, 2) and x.fence[0].numel() == G.GUARD * 8 and G.untouched(torch, x)
    assert G.ptr(x).value == x.fence[0].data_ptr()      # an empty buffer has an address too


# ---- 2. the shared checks against a stand-in renderer ----------------------------------------

class Schedule:
    def __init__(self, blocks, repeat):
        self.blocks, self.repeat, self.closed = blocks, repeat, False

    def order(self):
        o = list(range(self.blocks))[::-1]
        if self.repeat:
            o[0] = o[1]
        return o

    def close(self):
        self.closed = True


class StandIn:
    """Renderer.render on CPU tensors: the owned rows of a fixed random frame and
    steps array, packed or at their places.  `fault` names one mistake."""
    device = torch.device("cpu")

    def __init__(self, fault=None):
        rng = np.random.default_rng(5)
        self.rgba = torch.from_numpy(rng.random((H, W, 4), dtype=np.float32))
        self.steps = torch.from_numpy(rng.integers(1, 99, (H, W, 2), dtype=np.int32))
        self.fault = fault
        self.schedules = []

    def schedule(self, rows, period=1):
        self.schedules.append(Schedule((rows + 7) // 8, self.fault == "order repeats a block"))
        return self.schedules[-1]

    def render(self, frame, t=None, out=None, steps=False, schedule=None, **shading):
        assert set(shading) <= {"lights", "light_flags", "materials", "reflect", "env"}
        src = G.owned_row_index(H, t) if t is not None else np.arange(H)
        placed = t is not None and t.flags & abi.TILING_FRAME_ROWS
        dst = src if placed else np.arange(len(src))
        rgba = self.rgba.clone()
        if self.fault == "two owned rows swapped" and t is not None and len(src) > 1:
            rgba[[src[0], src[1]]] = rgba[[src[1], src[0]]]
        if self.fault == "colours depend on the steps buffer" and steps is not False:
            rgba[2, 3, 1] += 1.0
        if self.fault == "a scheduled render differs" and schedule is not None:
            rgba[H - 1, W - 1, 0] += 1.0
        out[dst] = rgba[src]
        if steps is not False:
            steps[dst] = self.steps[src]
        if self.fault == "a row past the end" and t is None:
            beyond = out.as_strided((out.shape[0] + 1, *out.shape[1:]), out.stride(),
                                    out.storage_offset())
            beyond[-1] = 0.5
        if self.fault == "an unowned row under FRAME_ROWS" and placed:
            other = np.setdiff1d(np.arange(H), src)
            out[other[0]] = rgba[other[0]]


def frame():
    return scenes.config("C3", W, H)


TILINGS = [(3, (1, 1)), (2, (1, 2))]


def test_helpers_pass_on_a_faultless_renderer():
    rd, f = StandIn(), frame()
    out, st = G.render(rd, f, lights=None, light_flags=0)
    assert G.same(out, rd.rgba.numpy()) and np.array_equal(st, rd.steps.numpy())
    out, none = G.render(rd, f, steps=False)
    assert G.same(out, rd.rgba.numpy()) and none is None
    out, st = G.both(rd, f, R.tiling(1, 2, 8))
    assert out.shape[0] == st.shape[0] == len(G.owned_row_index(H, R.tiling(1, 2, 8)))
    for world, shares in TILINGS:
        whole, whole_st = G.check_tilings(rd, f, world, shares, materials=None)
        assert G.same(whole, rd.rgba.numpy()) and np.array_equal(whole_st, rd.steps.numpy())
    ran = []
    G.check_scheduled(rd, f, after=ran.append, env=None)
    assert ran == rd.schedules and len(ran) == 1 and ran[0].closed
    G.check_formats(FormatStandIn(), f, rd.rgba.numpy())


class FormatStandIn(StandIn):
    """The stand-in with the output formats, converted as the library converts."""
    def render(self, frame, t=None, out=None, steps=False, schedule=None, **shading):
        from parity import quantize
        q = quantize(self.rgba.numpy(), frame.params.output_format)
        out.copy_(torch.from_numpy(np.ascontiguousarray(q)))
        if steps is not False:
            steps.copy_(self.steps)


@pytest.mark.parametrize("fault,helper", [
    ("a row past the end", "render"),
    ("an unowned row under FRAME_ROWS", "check_tilings"),
    ("two owned rows swapped", "check_tilings"),
    ("colours depend on the steps buffer", "both"),
    ("a scheduled render differs", "check_scheduled"),
    ("order repeats a block", "check_scheduled"),
])
def test_each_fault_is_caught_by_its_helper(fault, helper):
    f = frame()
    calls = {"render": lambda rd: [G.render(rd, f)],
             "both": lambda rd: [G.both(rd, f)],
             "check_tilings": lambda rd: [G.check_tilings(rd, f, w, s) for w, s in TILINGS[:1]],
             "check_scheduled": lambda rd: [G.check_scheduled(rd, f)]}
    calls[helper](StandIn())                      # passes without the fault
    with pytest.raises(AssertionError) as e:
        calls[helper](StandIn(fault))
    assert str(e.value), "an assertion of the support module without a message"
    if helper == "check_tilings":                 # and under the other tiling too
        with pytest.raises(AssertionError):
            G.check_tilings(StandIn(fault), f, *TILINGS[1])
    if helper == "check_scheduled":               # the schedule is closed all the same
        rd = StandIn(fault)
        with pytest.raises(AssertionError):
            G.check_scheduled(rd, f)
        assert rd.schedules[0].closed


def test_format_fault_is_caught():
    class Wrong(FormatStandIn):
        def render(self, frame, t=None, out=None, steps=False, schedule=None, **shading):
            super().render(frame, t, out, steps, schedule, **shading)
            if frame.params.output_format == abi.FORMAT_RGBA8:
                out[0, 0, 0] += 1
    with pytest.raises(AssertionError):
        G.check_formats(Wrong(), frame(), StandIn().rgba.numpy())


def test_own_layers_on_frames_and_ray_lists():
    """The layer axis is -2 in both layouts, and each assertion of the copies is
    there: equal steps of the colour and the weight pass, alpha 1, zeros on the
    layers a path did not reach."""
    rng = np.random.default_rng(9)

    def kernel(shape, fault=None):
        reach = rng.integers(0, 3, shape)          # the last layer a path reaches
        def call(r):
            alive = r.layer <= reach
            st = np.where(alive[..., None], np.int32(r.layer + 1), np.int32(0)) * np.ones(2, np.int32)
            rgba = np.ones(shape + (4,), np.float32)
            value = 0.25 if r.flags & abi.REFLECT_WEIGHT else 0.5
            rgba[..., :3] = np.where(alive[..., None], np.float32(value), np.float32(0))
            if fault == "steps" and r.flags & abi.REFLECT_WEIGHT:
                st = st + 1
            if fault == "alpha":
                rgba[..., 3] = 0.5
            if fault == "dead colour" and not r.flags & abi.REFLECT_WEIGHT:
                rgba[..., :3] = 0.5
            return rgba, st.astype(np.int32)
        return call, reach

    for shape in ((H, W), (W * H,)):
        call, reach = kernel(shape)
        Cj, Wj, Sj, alive = G.own_layers(call, 2, 1.0)
        assert Cj.shape == Wj.shape == shape + (3, 3) and Sj.shape == shape + (3, 2)
        assert np.array_equal(alive, np.arange(3) <= reach[..., None])
        for fault in ("steps", "alpha", "dead colour"):
            with pytest.raises(AssertionError):
                G.own_layers(kernel(shape, fault)[0], 2, 1.0)


def test_comparisons():
    a = np.array([1.0, np.nan, -0.0], np.float32)
    assert G.same(a, a.copy()) and not G.same(a, a.astype(np.float64)) and not G.same(a, a[:2])
    assert G.ndiff(a, np.array([1.0, np.nan, 0.0], np.float32)) == 1
    assert G.bitwise_eq(a, a.copy()).all()
    other_nan = a.copy()
    other_nan.view(np.uint32)[1] ^= 1             # another NaN: equal elementwise, not in bytes
    assert G.bitwise_eq(a, other_nan).all() and not G.same(a, other_nan)
    assert list(G.bitwise_eq(a, np.array([1.0, np.nan, 0.0], np.float32))) == [True, True, False]
    with pytest.raises(AssertionError):
        G.ndiff(a, a[:2])


# ---- 3. the counted signatures ---------------------------------------------------------------

def test_counted_scenes_have_signatures_of_their_own():
    """Pairwise distinct among the scenes whose compilations a test counts, the
    run-time specialised scenes used beside them and C4-carved, and none the
    sequence of a built-in scene (taken from the scene structs)."""
    built_in = {name: cases.signature(scenes.config(name, 64, 36).scene)
                for name in ("REF", "C1", "C2", "C3", "C4")}
    assert len(set(built_in.values())) == 3      # the built-in variants 1, 2 and 3
    jit = {**cases.COUNTED, **cases.UNCOUNTED, "fast_paths: C4-carved": FP.PATHS["C4-carved"]}
    assert {f"query, mesh: {k}" for k in cases.JIT_SEEDS} <= set(cases.COUNTED)
    sig = {}
    for name, build in jit.items():
        f = build()
        assert f.scene.kind == abi.SCENE_PRIMITIVES, name
        assert f.params.dispatch == abi.DISPATCH_AUTO, name
        sig[name] = cases.signature(f.scene)
    for name, s in sig.items():
        assert s not in built_in.values(), f"{name} is a built-in variant's sequence"
        twins = [other for other, t in sig.items() if t == s and other != name]
        assert not twins, f"{name} shares its sequence with {twins}"


def test_seeded_custom_scenes_are_the_jit_tests():
    for k, seed in cases.JIT_SEEDS.items():
        a = cases.query_frame(k).scene
        b = cases.custom_scene(np.random.default_rng(100 + seed), 2 + seed % 7).scene
        assert cases.signature(a) == cases.signature(b) and a.count == 3 + seed % 7
