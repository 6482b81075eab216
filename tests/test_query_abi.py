"""The query entry points at the C-ABI boundary, without a device
(include/sdf_abi.h "Queries"): the symbols exist, sdf_hits has its layout, the
validator rejects what it must, every SDF_E_INVALID_ARG case is decided before
any device call, and n = 0 is SDF_OK on a machine with no GPU."""
import ctypes as C

import pytest

from sdf3d_amd import abi, scenes

OK, INVALID, UNSUPPORTED = abi.SDF_OK, abi.SDF_E_INVALID_ARG, abi.SDF_E_UNSUPPORTED
PTR = 0x1000   # a non-null "device pointer": never dereferenced before a device call


@pytest.fixture(scope="module")
def lib():
    return abi.load_library()


def frame(name="C4"):
    return scenes.config(name, 64, 36)


def hits(t=PTR, steps=None, normal=None, prim=None):
    return abi.sdf_hits(t, steps, normal, prim)


def trace(lib, f, origins=PTR, dirs=PTR, n=1, h=None, scene=True, params=True):
    h = hits() if h is None else h
    return lib.sdf_trace(C.byref(f.scene) if scene else None,
                         C.byref(f.params) if params else None, origins, dirs, n,
                         C.byref(h) if h is not False else None, None)


def sample(lib, f, points=PTR, n=1, dist=PTR, normal=None):
    return lib.sdf_sample(C.byref(f.scene), C.byref(f.params), points, n, dist, normal, None)


def test_symbols_and_layout(lib):
    for name in ("sdf_validate_query", "sdf_trace", "sdf_trace_camera", "sdf_sample"):
        assert hasattr(lib, name), name
        assert name in abi.SIGNATURES
    assert C.sizeof(abi.sdf_hits) == 32 == abi.STRUCT_SIZES["sdf_hits"]
    assert lib.sdf_abi_version() == 12 == abi.SDF_ABI_VERSION


def test_validator_accepts_every_config(lib):
    for name in scenes.CONFIGS:
        f = scenes.config(name)
        assert lib.sdf_validate_query(C.byref(f.scene), C.byref(f.params)) == OK, name


def test_validator_rejections(lib):
    f = frame()
    assert lib.sdf_validate_query(None, C.byref(f.params)) == INVALID
    assert lib.sdf_validate_query(C.byref(f.scene), None) == INVALID
    for field, bad in [("max_steps", -1), ("max_steps", (1 << 24) + 1), ("max_dist", float("nan")),
                       ("max_dist", 1e16), ("eps", float("inf")), ("normal_eps", float("nan")),
                       ("normal_mode", 2), ("precision", 2), ("dispatch", 3), ("dispatch", -1)]:
        g = f.copy()
        setattr(g.params, field, bad)
        assert lib.sdf_validate_query(C.byref(g.scene), C.byref(g.params)) == INVALID, field
    # the scene checks are sdf_validate's
    g = f.copy()
    g.scene.count = abi.SDF_MAX_PRIMS + 1
    assert lib.sdf_validate_query(C.byref(g.scene), C.byref(g.params)) == INVALID
    g = f.copy()
    g.scene.prims[1].k = 0.0                      # a smooth union without a radius
    assert lib.sdf_validate_query(C.byref(g.scene), C.byref(g.params)) == INVALID
    g = f.copy()
    g.scene.prims[2].p[0] = float("nan")
    assert lib.sdf_validate_query(C.byref(g.scene), C.byref(g.params)) == INVALID
    g = frame("C5")
    g.scene.bulb_iterations = 0
    assert lib.sdf_validate_query(C.byref(g.scene), C.byref(g.params)) == INVALID


def test_ignored_fields_are_ignored(lib):
    """Fields a query does not use cannot fail it: the copy that is validated
    carries sdf_defaults' values there."""
    f = frame()
    p = f.params
    p.width = p.height = -5
    p.flags = 0x7fff
    p.ao_taps = 10 ** 6
    p.shadow_k = float("nan")
    p.shadow_offset = float("inf")
    p.output_format = 99
    p.samples = 3
    assert lib.sdf_validate_query(C.byref(f.scene), C.byref(p)) == OK
    assert trace(lib, f, n=0) == OK
    assert sample(lib, f, n=0) == OK


def test_invalid_arguments_before_any_device_call(lib):
    f = frame()
    assert trace(lib, f, scene=False) == INVALID
    assert trace(lib, f, params=False) == INVALID
    assert trace(lib, f, h=False) == INVALID
    assert trace(lib, f, h=hits(None)) == INVALID                 # every output NULL
    assert trace(lib, f, origins=None) == INVALID
    assert trace(lib, f, dirs=None) == INVALID
    assert trace(lib, f, n=-1) == INVALID
    assert trace(lib, f, n=(1 << 30) + 1) == INVALID
    g = f.copy()
    g.params.max_steps = -1
    assert trace(lib, g) == INVALID and trace(lib, g, n=0) == INVALID
    assert sample(lib, f, points=None) == INVALID
    assert sample(lib, f, dist=None, normal=None) == INVALID
    assert sample(lib, f, n=-1) == INVALID
    assert sample(lib, f, n=(1 << 30) + 1) == INVALID
    assert sample(lib, g) == INVALID
    assert lib.sdf_sample(None, C.byref(f.params), PTR, 1, PTR, None, None) == INVALID
    assert lib.sdf_sample(C.byref(f.scene), None, PTR, 1, PTR, None, None) == INVALID
    h = hits()
    cam = lambda scene=True, camera=True, params=True, hh=h, fr=f: lib.sdf_trace_camera(
        C.byref(fr.scene) if scene else None, C.byref(fr.camera) if camera else None,
        C.byref(fr.params) if params else None, C.byref(hh) if hh is not None else None, None)
    assert cam(scene=False) == INVALID
    assert cam(camera=False) == INVALID
    assert cam(params=False) == INVALID
    assert cam(hh=None) == INVALID
    assert cam(hh=hits(None)) == INVALID
    w = f.copy()
    w.params.width = 0
    assert cam(fr=w) == INVALID
    w = f.copy()
    w.camera.eye[0] = float("nan")
    assert cam(fr=w) == INVALID
    assert cam(fr=g) == INVALID
    s = f.copy()
    s.params.samples = 2
    assert cam(fr=s) == UNSUPPORTED


def test_nothing_to_do_needs_no_device(lib):
    """n = 0 launches nothing and touches no buffer: SDF_OK without a GPU, with
    null inputs too."""
    for name in ("REF", "C4", "C5"):
        f = frame(name)
        assert trace(lib, f, n=0) == OK
        assert trace(lib, f, origins=None, dirs=None, n=0) == OK
        assert sample(lib, f, n=0) == OK
        assert sample(lib, f, points=None, n=0) == OK


def test_renderer_checks_its_tensors():
    """Renderer.trace / sample refuse anything but contiguous float32 (n, 3)
    tensors on the device, before any call (a stand-in renderer: no GPU)."""
    import torch
    from sdf3d_amd.renderer import Renderer
    rd = Renderer.__new__(Renderer)
    rd.torch, rd.device, rd.lib = torch, torch.device("cpu"), None
    f = frame()
    good = torch.zeros((4, 3), dtype=torch.float32)
    for bad in (good.double(), torch.zeros((4, 4)), torch.zeros((3, 4)).t(), torch.zeros(12),
                good.numpy()):
        with pytest.raises(ValueError):
            rd.trace(f, bad, good)
        with pytest.raises(ValueError):
            rd.trace(f, good, bad)
        with pytest.raises(ValueError):
            rd.sample(f, bad)
    with pytest.raises(ValueError):
        rd.trace(f, good, torch.zeros((5, 3)))
    with pytest.raises(ValueError):
        rd.trace(f, good, good, normal=False, prim=False, t=False, steps=False)
