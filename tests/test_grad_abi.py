"""The gradient entry points at the C-ABI boundary, without a GPU (include/
sdf_abi.h "Gradients"): symbols and layouts, every documented error decided
before any device call, n = 0, the workspace formula, and the scene <-> tensor
round trip of sdf3d_amd/autograd.py."""
import ctypes as C

import numpy as np
import pytest

from sdf3d_amd import abi, scenes

INVALID = abi.SDF_E_INVALID_ARG
FAKE = C.c_void_p(1 << 20)          # a 16-byte aligned address that is never dereferenced
ODD = C.c_void_p((1 << 20) + 4)     # not 16-byte aligned


@pytest.fixture(scope="module")
def lib():
    return abi.load_library()


def frame(name="C4"):
    return scenes.config(name, 64, 36)


def call(lib, f, n=100, points=FAKE, upstream=None, out="all", ws=FAKE, nbytes=None):
    if nbytes is None:
        nbytes = max(int(lib.sdf_grad_workspace_bytes(n)), 0)
    if out == "all":
        out = abi.sdf_grad_out(FAKE, FAKE, FAKE)
    return lib.sdf_sample_grad(C.byref(f.scene), C.byref(f.params), points, n, upstream,
                               C.byref(out) if out is not None else None, ws, nbytes, None)


def test_symbols_and_layout(lib):
    for name, nargs in (("sdf_validate_grad", 2), ("sdf_grad_workspace_bytes", 1),
                        ("sdf_sample_grad", 9)):
        assert hasattr(lib, name), name
        assert len(abi.SIGNATURES[name][1]) == nargs
    assert abi.SIGNATURES["sdf_grad_workspace_bytes"][0] is C.c_int64
    assert C.sizeof(abi.sdf_grad_out) == 24 == abi.STRUCT_SIZES["sdf_grad_out"]
    assert [n for n, _ in abi.sdf_grad_out._fields_] == ["dist", "grad_points", "grad_prims"]
    assert lib.sdf_abi_version() == 12 == abi.SDF_ABI_VERSION


def test_validator(lib):
    for name in scenes.CONFIGS:
        f = scenes.config(name)
        want = abi.SDF_E_UNSUPPORTED if name == "C5" else abi.SDF_OK
        assert lib.sdf_validate_grad(C.byref(f.scene), C.byref(f.params)) == want, name
    f = frame()
    assert lib.sdf_validate_grad(None, C.byref(f.params)) == INVALID
    assert lib.sdf_validate_grad(C.byref(f.scene), None) == INVALID
    # everything sdf_validate_query rejects
    for edit in (lambda f: setattr(f.params, "precision", 7),
                 lambda f: setattr(f.params, "dispatch", 9),
                 lambda f: setattr(f.scene, "count", abi.SDF_MAX_PRIMS + 1),
                 lambda f: setattr(f.scene.prims[1], "kind", 99),
                 lambda f: setattr(f.scene.prims[1], "k", 0.0)):
        g = frame()
        edit(g)
        assert lib.sdf_validate_query(C.byref(g.scene), C.byref(g.params)) == INVALID
        assert lib.sdf_validate_grad(C.byref(g.scene), C.byref(g.params)) == INVALID
        assert call(lib, g) == INVALID
        assert call(lib, g, n=0) == INVALID


def test_invalid_arguments_before_any_device_call(lib):
    f = frame()
    assert call(lib, f, out=None) == INVALID
    assert call(lib, f, out=abi.sdf_grad_out(None, None, None)) == INVALID
    assert call(lib, f, points=None) == INVALID
    assert call(lib, f, n=-1, nbytes=1 << 20) == INVALID
    assert call(lib, f, n=(1 << 30) + 1, nbytes=1 << 20) == INVALID
    assert lib.sdf_sample_grad(None, C.byref(f.params), FAKE, 10, None,
                               C.byref(abi.sdf_grad_out(FAKE, None, None)), None, 0, None) == INVALID
    assert lib.sdf_sample_grad(C.byref(f.scene), None, FAKE, 10, None,
                               C.byref(abi.sdf_grad_out(FAKE, None, None)), None, 0, None) == INVALID
    # grad_prims needs its workspace: present, aligned, large enough
    need = int(lib.sdf_grad_workspace_bytes(100))
    assert need > 0
    assert call(lib, f, ws=None) == INVALID
    assert call(lib, f, ws=ODD) == INVALID
    assert call(lib, f, nbytes=need - 1) == INVALID
    assert call(lib, f, nbytes=0) == INVALID


def test_mandelbulb_is_unsupported(lib):
    f = frame("C5")
    assert call(lib, f) == abi.SDF_E_UNSUPPORTED
    assert call(lib, f, out=abi.sdf_grad_out(None, FAKE, None), ws=None, nbytes=0) == \
        abi.SDF_E_UNSUPPORTED
    # an invalid argument is reported first
    assert call(lib, f, points=None) == INVALID


def test_n_zero_touches_nothing(lib):
    f = frame()
    bufs = [np.full(256, 12345.0, dtype=np.float32) for _ in range(5)]
    ptr = [C.c_void_p(b.ctypes.data) for b in bufs]
    out = abi.sdf_grad_out(ptr[0], ptr[1], ptr[2])
    rc = lib.sdf_sample_grad(C.byref(f.scene), C.byref(f.params), ptr[3], 0, ptr[4], C.byref(out),
                             None, 0, None)
    assert rc == abi.SDF_OK
    assert call(lib, f, n=0, points=None, ws=None, nbytes=0) == abi.SDF_OK
    for b in bufs:
        assert np.all(b == 12345.0)


def test_workspace_bytes(lib):
    w = lib.sdf_grad_workspace_bytes
    assert w(0) == 0
    assert w(-1) < 0 and w(-(1 << 40)) < 0 and w((1 << 30) + 1) < 0
    ns = [1, 2, 63, 64, 65, 255, 256, 257, 1000, 1 << 12, 1 << 16, (1 << 18) - 1, 1 << 18,
          (1 << 18) + 7, 1 << 20, 1 << 25, 1 << 30]
    sizes = [int(w(n)) for n in ns]
    assert all(s > 0 and s % 16 == 0 for s in sizes)
    assert sizes == sorted(sizes)                  # monotone in n
    assert sizes[-1] <= 1 << 20                    # bounded: the grid is capped
    assert sizes[0] == 1024 and int(w(257)) == 2048    # one 256-float row per 256 points


def test_scene_tensor_round_trip():
    from sdf3d_amd import autograd as ag
    import torch
    for name in ("REF", "C1", "C4"):
        f = frame(name)
        # a reserved slot and an unused parameter slot must survive as well
        f.scene.prims[0].reserved = 0.75
        f.scene.prims[0].p[11] = -3.5
        th = ag.scene_tensor(f.scene)
        n = f.scene.count
        assert tuple(th.shape) == (n, 16) and th.dtype == torch.float32
        for i in range(n):
            assert th[i, 0] == f.scene.prims[i].kind and th[i, 1] == f.scene.prims[i].op
            assert th[i, 2] == f.scene.prims[i].k
        back = ag.apply(f.scene, th)
        assert bytes(back) == bytes(f.scene)
        # the kind and op slots of theta are never written back
        th2 = th.clone()
        th2[:, 0:2] = 77.0
        assert bytes(ag.apply(f.scene, th2)) == bytes(f.scene)
        # a float slot is
        th3 = th.clone()
        th3[0, 4] = 0.125
        moved = ag.apply(f.scene, th3)
        assert moved.prims[0].p[0] == 0.125 and bytes(moved) != bytes(f.scene)
        assert moved.prims[0].kind == f.scene.prims[0].kind
    with pytest.raises(ValueError):
        ag.apply(frame().scene, torch.zeros((3, 16)))
