"""Supersampling (sdf_params.samples) at the C-ABI boundary, without a GPU:
what sdf_validate accepts and refuses, the entry points that do not serve it,
the unchanged struct layout, and the NumPy statement of the resolve
(tests/ssaa_ref.py) that the GPU tests hold the kernels to."""
import ctypes as C

import numpy as np
import pytest

import ssaa_ref
from sdf3d_amd import abi, renderer as R, scenes


def _validate(f, t=None):
    lib = abi.load_library()
    return lib.sdf_validate(C.byref(f.scene), C.byref(f.camera), C.byref(f.light),
                            C.byref(f.material), C.byref(f.params),
                            C.byref(t) if t is not None else None)


@pytest.mark.parametrize("name", sorted(scenes.CONFIGS))
@pytest.mark.parametrize("samples", [0, 1, 2, 4])
def test_validate_accepts_samples(name, samples):
    f = scenes.config(name)
    f.params.samples = samples
    assert _validate(f) == abi.SDF_OK


@pytest.mark.parametrize("samples", [3, 8, -1])
def test_validate_rejects_other_sample_counts(samples):
    f = scenes.reference()
    f.params.samples = samples
    assert _validate(f) == abi.SDF_E_INVALID_ARG


def test_validate_bounds_the_subsample_frame():
    """samples * width and samples * height stay within the kernels' 65536."""
    f = scenes.reference(40000, 16)
    assert _validate(f) == abi.SDF_OK
    f.params.samples = 2
    assert _validate(f) == abi.SDF_E_INVALID_ARG
    f = scenes.reference(16, 40000)
    f.params.samples = 2
    assert _validate(f) == abi.SDF_E_INVALID_ARG
    f = scenes.reference(32768, 16384)
    f.params.samples = 2
    assert _validate(f) == abi.SDF_OK
    f.params.samples = 4
    assert _validate(f) == abi.SDF_E_INVALID_ARG
    # the scaled tiling's block_rows must fit an int32
    f = scenes.reference(64, 64)
    f.params.samples = 4
    t = R.tiling(block_rows=1 << 30)
    assert _validate(f, t) == abi.SDF_E_INVALID_ARG
    f.params.samples = 1
    assert _validate(f, t) == abi.SDF_OK


@pytest.mark.parametrize("fmt", [abi.FORMAT_TILES, abi.FORMAT_SHADE32F])
def test_validate_terms_formats_are_unsupported(fmt):
    """Shading terms do not average to the colour."""
    f = scenes.config("C3", 64, 40)
    f.params.output_format = fmt
    for s in (0, 1):
        f.params.samples = s
        assert _validate(f) == abi.SDF_OK
    f.params.samples = 2
    assert _validate(f) == abi.SDF_E_UNSUPPORTED
    f.params.samples = 3                      # a bad value stays a bad value
    assert _validate(f) == abi.SDF_E_INVALID_ARG


def test_defaults_leave_samples_zero_and_layout_unchanged():
    f = scenes.reference(37, 23)
    assert f.params.samples == 0 and f.params.reserved[0] == 0
    assert C.sizeof(abi.sdf_params) == 80 == abi.STRUCT_SIZES["sdf_params"]
    assert abi.sdf_params.samples.offset == 72 and abi.sdf_params.samples.size == 4
    assert abi.sdf_params.output_format.offset == 68
    assert abi.SDF_ABI_VERSION == 12 == abi.load_library().sdf_abi_version()


def test_other_entry_points_refuse_supersampling_without_a_device():
    """sdf_render_frames, sdf_render_multi and sdf_driver_create decide it
    before any device call (and before they look at their buffers)."""
    lib = abi.load_library()
    f = scenes.config("C3", 64, 40)
    f.params.samples = 2
    fr = (C.byref(f.scene), C.byref(f.camera), C.byref(f.light), C.byref(f.material),
          C.byref(f.params))
    # never dereferenced: the calls return before touching them
    fake = C.c_void_p(0x1000)
    ptrs = (C.c_void_p * 1)(fake)
    cams = (abi.sdf_camera * 1)(f.camera)
    assert lib.sdf_render_frames(C.byref(f.scene), cams, 1, C.byref(f.light),
                                 C.byref(f.material), C.byref(f.params), ptrs, None,
                                 None) == abi.SDF_E_UNSUPPORTED
    devs = (C.c_int32 * 1)(0)
    assert lib.sdf_render_multi(*fr, 1, devs, 1, 1, fake, None) == abi.SDF_E_UNSUPPORTED
    for world in (1, 2):
        cfg = abi.sdf_driver_config(rank=0, world=world, share_root=1, share_peer=1, nbuf=3,
                                    lag=1, flags=0, timeout_ms=1000, batch=1)
        drv = C.c_void_p()
        assert lib.sdf_driver_create(*fr, C.byref(cfg), None, None,
                                     C.byref(drv)) == abi.SDF_E_UNSUPPORTED
        assert not drv.value


def test_steps_shape_scales_with_samples():
    f = scenes.reference(37, 23)
    assert R.steps_shape(f) == (23, 37, 2)
    f.params.samples = 1
    assert R.steps_shape(f) == (23, 37, 2)
    f.params.samples = 2
    assert R.steps_shape(f) == (46, 74, 2)
    t = R.tiling(1, 2)                        # rows 8..15 of 23
    assert R.steps_shape(f, t) == (16, 74, 2)
    t = R.tiling(1, 2, frame_rows=True)
    f.params.samples = 4
    assert R.steps_shape(f, t) == (92, 148, 2)


# ---- the reference resolve ---------------------------------------------------

def _group(vals, s):
    """A one-pixel S x S frame whose sub-sample (i, j) carries vals[j][i] in
    R, twice that in G and its negative in B."""
    a = np.zeros((s, s, 4), dtype=np.float32)
    v = np.asarray(vals, dtype=np.float32)
    a[..., 0], a[..., 1], a[..., 2], a[..., 3] = v, 2 * v, -v, 1.0
    return a


def test_resolve_2x2_tree_order():
    # rows j (y), columns i (x); tree: (1 + 2^-24) -> 1, (2^-24 + 2^-24) = 2^-23
    e = 2.0 ** -24
    g = _group([[1.0, e], [e, e]], 2)
    tree = np.float32((np.float32(np.float32(1.0) + np.float32(e)) +
                       np.float32(np.float32(e) + np.float32(e))) * np.float32(0.25))
    assert tree == np.float32((1.0 + 2.0 ** -23) * 0.25)
    out = ssaa_ref.resolve(g, 2)
    assert out.shape == (1, 1, 4) and out.dtype == np.float32
    assert out[0, 0, 0] == tree and out[0, 0, 1] == 2 * tree and out[0, 0, 2] == -tree
    assert out[0, 0, 3] == 1.0
    seq = ssaa_ref.resolve_sequential(g, 2)           # ((1 + e) + e) + e = 1
    assert seq[0, 0, 0] == np.float32(0.25) != out[0, 0, 0]
    # x first, then y: transposing the group changes the pairing
    gt = _group([[1.0, e], [2 * e, -e]], 2)
    assert ssaa_ref.resolve(gt, 2)[0, 0, 0] != ssaa_ref.resolve(
        np.ascontiguousarray(gt.transpose(1, 0, 2)), 2)[0, 0, 0]


def test_resolve_4x4_tree_order():
    e = np.float32(2.0 ** -24)
    vals = np.full((4, 4), e, dtype=np.float32)
    vals[0, 0] = 1.0
    g = _group(vals, 4)
    f32 = np.float32
    rows = []
    for j in range(4):
        c = vals[j]
        rows.append(f32(f32(c[0] + c[1]) + f32(c[2] + c[3])))
    tree = f32(f32(f32(rows[0] + rows[1]) + f32(rows[2] + rows[3])) * f32(0.0625))
    out = ssaa_ref.resolve(g, 4)
    assert out.shape == (1, 1, 4)
    assert out[0, 0, 0] == tree
    # the tree keeps the 15 small terms (pairs of them are representable
    # beside 1), the sequential sum drops every one
    assert tree == f32((1.0 + 14 * 2.0 ** -24) * 0.0625)
    assert ssaa_ref.resolve_sequential(g, 4)[0, 0, 0] == f32(0.0625)


def test_resolve_keeps_denormals():
    tiny = np.float32(2.0 ** -126)                   # the smallest normal
    g = _group([[tiny, 0.0], [0.0, 0.0]], 2)
    out = ssaa_ref.resolve(g, 2)
    assert out[0, 0, 0] == np.float32(2.0 ** -128) and out[0, 0, 0] != 0.0
    sub = np.float32(3 * 2.0 ** -149)                # a subnormal input
    g = _group([[sub, sub], [sub, sub]], 2)
    assert ssaa_ref.resolve(g, 2)[0, 0, 0] == sub
    g = _group(np.full((4, 4), sub), 4)
    assert ssaa_ref.resolve(g, 4)[0, 0, 0] == sub
    # 2^-149 / 4 lies below half the smallest subnormal: it rounds to +0
    one = np.float32(2.0 ** -149)
    assert ssaa_ref.resolve(_group([[one, 0.0], [0.0, 0.0]], 2), 2)[0, 0, 0] == 0.0


@pytest.mark.parametrize("s", [2, 4])
def test_resolve_agrees_with_fp64_mean(s):
    """Every addition and the scaling round once: S^2 - 1 additions in a tree
    of depth 2 log2 S, so the result is within (2 log2 S + 1) 2^-24 of the
    exact mean of positive data, relatively."""
    rng = np.random.default_rng(5)
    hi = rng.random((6 * s, 10 * s, 4), dtype=np.float32)
    hi[..., 3] = 1.0
    out = ssaa_ref.resolve(hi, s)
    mean = hi.astype(np.float64).reshape(6, s, 10, s, 4).mean(axis=(1, 3))
    depth = 2 * (1 if s == 2 else 2)
    rel = np.abs(out[..., :3].astype(np.float64) - mean[..., :3]) / mean[..., :3]
    assert rel.max() <= (depth + 1) * 2.0 ** -24
    assert np.all(out[..., 3] == 1.0)
    # and the order is visible on ordinary data, too
    seq = ssaa_ref.resolve_sequential(hi, s)
    assert (seq[..., :3] != out[..., :3]).any()


def test_resolve_identity_and_errors():
    hi = np.arange(2 * 4 * 4, dtype=np.float32).reshape(2, 4, 4)
    assert np.array_equal(ssaa_ref.resolve(hi, 0), hi) and np.array_equal(ssaa_ref.resolve(hi, 1), hi)
    with pytest.raises(ValueError):
        ssaa_ref.resolve(hi, 3)
    with pytest.raises(ValueError):
        ssaa_ref.resolve(hi[:1], 2)
