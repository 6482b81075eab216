"""The mesh entry points at the C-ABI boundary, without a GPU (include/sdf_abi.h
"Meshes"): symbols and layouts, every documented error decided before any
device call, the workspace formula, and the OBJ writer and reader."""
import ctypes as C
import math

import numpy as np
import pytest

from sdf3d_amd import abi, meshio, renderer as R, scenes

INVALID = abi.SDF_E_INVALID_ARG
FAKE = C.c_void_p(1 << 20)          # a 16-byte aligned address that is never dereferenced


@pytest.fixture(scope="module")
def lib():
    return abi.load_library()


def frame():
    return scenes.config("C4", 64, 36)


def good_grid():
    return R.grid((-1.13, -0.11, -1.02), (0.12, 0.08, 0.11), (19, 11, 17))


def calls(lib, f, g, ws=FAKE, nbytes=None, counts=FAKE, out=None):
    """(validate, count, emit) return codes for one set of arguments."""
    if nbytes is None:
        nbytes = max(int(lib.sdf_mesh_workspace_bytes(C.byref(g))), 0) if g is not None else 0
    o = abi.sdf_mesh_out(FAKE, 10, FAKE, 10, None, None) if out is None else out
    gp = C.byref(g) if g is not None else None
    return (lib.sdf_validate_mesh(C.byref(f.scene), C.byref(f.params), gp),
            lib.sdf_mesh_count(C.byref(f.scene), C.byref(f.params), gp, ws, nbytes, counts, None),
            lib.sdf_mesh_emit(C.byref(f.scene), C.byref(f.params), gp, ws, nbytes, C.byref(o), None))


def test_symbols_and_layout(lib):
    for name, nargs in (("sdf_validate_mesh", 3), ("sdf_mesh_workspace_bytes", 1),
                        ("sdf_mesh_count", 7), ("sdf_mesh_emit", 7)):
        assert hasattr(lib, name), name
        assert len(abi.SIGNATURES[name][1]) == nargs
    assert abi.SIGNATURES["sdf_mesh_workspace_bytes"][0] is C.c_int64
    assert C.sizeof(abi.sdf_grid) == 48 == abi.STRUCT_SIZES["sdf_grid"]
    assert C.sizeof(abi.sdf_mesh_out) == 48 == abi.STRUCT_SIZES["sdf_mesh_out"]
    assert [n for n, _ in abi.sdf_grid._fields_] == ["origin", "cell", "n", "iso", "flags", "reserved"]
    assert abi.sdf_grid.iso.offset == 36 and abi.sdf_mesh_out.max_tris.offset == 24
    assert abi.MESH_DENSE == 1
    assert lib.sdf_abi_version() == 12 == abi.SDF_ABI_VERSION


def test_validator_accepts_every_config(lib):
    g = good_grid()
    for name in scenes.CONFIGS:
        f = scenes.config(name)
        assert lib.sdf_validate_mesh(C.byref(f.scene), C.byref(f.params), C.byref(g)) == abi.SDF_OK
    g.flags = abi.MESH_DENSE
    g.iso = 0.05
    f = frame()
    assert lib.sdf_validate_mesh(C.byref(f.scene), C.byref(f.params), C.byref(g)) == abi.SDF_OK


def bad_grids():
    def edit(**kw):
        g = good_grid()
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(g, k)[v[0]] = v[1]
            else:
                setattr(g, k, v)
        return g
    inf, nan = math.inf, math.nan
    return {
        "n zero": edit(n=(1, 0)), "n negative": edit(n=(2, -3)),
        "too many lattice points": edit(n=(0, 1 << 30)),
        "2^30 + 1 points": R.grid((0, 0, 0), 0.001, (1023, 1023, 1024)),
        "cell zero": edit(cell=(0, 0.0)), "cell negative": edit(cell=(1, -0.1)),
        "cell inf": edit(cell=(2, inf)), "cell nan": edit(cell=(0, nan)),
        "origin nan": edit(origin=(1, nan)), "origin inf": edit(origin=(0, -inf)),
        "origin beyond 1e15": edit(origin=(2, 2e15)),
        "iso nan": edit(iso=nan), "iso inf": edit(iso=inf), "iso beyond 1e15": edit(iso=-2e15),
        "far corner beyond 1e15": R.grid((9.9e14, 0, 0), (1e12, 1.0, 1.0), (19, 2, 2)),
        "unknown flag": edit(flags=2), "reserved": edit(reserved=1),
    }


@pytest.mark.parametrize("what", list(bad_grids()))
def test_bad_grids_are_refused(lib, what):
    g = bad_grids()[what]
    assert calls(lib, frame(), g) == (INVALID, INVALID, INVALID)
    assert lib.sdf_mesh_workspace_bytes(C.byref(g)) == INVALID


def test_largest_lattice_is_accepted(lib):
    g = R.grid((0, 0, 0), 0.001, (1023, 1023, 1023))          # exactly 2^30 points
    f = frame()
    assert lib.sdf_validate_mesh(C.byref(f.scene), C.byref(f.params), C.byref(g)) == abi.SDF_OK


def test_null_arguments_and_buffers(lib):
    f, g = frame(), good_grid()
    need = int(lib.sdf_mesh_workspace_bytes(C.byref(g)))
    assert calls(lib, f, None) == (INVALID, INVALID, INVALID)
    assert lib.sdf_mesh_workspace_bytes(None) == INVALID
    assert lib.sdf_validate_mesh(None, C.byref(f.params), C.byref(g)) == INVALID
    assert lib.sdf_validate_mesh(C.byref(f.scene), None, C.byref(g)) == INVALID
    assert calls(lib, f, g, ws=None)[1:] == (INVALID, INVALID)
    assert calls(lib, f, g, nbytes=need - 1)[1:] == (INVALID, INVALID)
    assert calls(lib, f, g, ws=C.c_void_p((1 << 20) + 8))[1:] == (INVALID, INVALID)   # misaligned
    assert lib.sdf_mesh_count(C.byref(f.scene), C.byref(f.params), C.byref(g), FAKE, need, None,
                              None) == INVALID
    emit = lambda o: lib.sdf_mesh_emit(C.byref(f.scene), C.byref(f.params), C.byref(g), FAKE, need,
                                       C.byref(o) if o is not None else None, None)
    assert emit(None) == INVALID
    assert emit(abi.sdf_mesh_out(None, 5, FAKE, 5, None, None)) == INVALID
    assert emit(abi.sdf_mesh_out(FAKE, 5, None, 5, None, None)) == INVALID
    assert emit(abi.sdf_mesh_out(FAKE, -1, FAKE, 5, None, None)) == INVALID
    assert emit(abi.sdf_mesh_out(FAKE, 5, FAKE, -1, None, None)) == INVALID
    # capacities of 0 with NULL buffers: nothing to write, nothing launched, no device needed
    assert emit(abi.sdf_mesh_out(None, 0, None, 0, None, None)) == abi.SDF_OK


def test_what_the_query_validator_rejects(lib):
    g = good_grid()
    f = frame()
    f.params.normal_mode = 7
    assert calls(lib, f, g) == (INVALID, INVALID, INVALID)
    f = frame()
    f.params.precision = 9
    assert calls(lib, f, g) == (INVALID, INVALID, INVALID)
    f = frame()
    f.scene.prims[1].kind = 99
    assert calls(lib, f, g) == (INVALID, INVALID, INVALID)
    f = frame()
    f.params.flags = 0x40            # a field the mesh does not use is not validated
    assert lib.sdf_validate_mesh(C.byref(f.scene), C.byref(f.params), C.byref(g)) == abi.SDF_OK


def test_workspace_is_per_brick(lib):
    def need(n):
        return int(lib.sdf_mesh_workspace_bytes(C.byref(R.grid((0, 0, 0), 0.01, n))))

    def formula(n):
        b = math.prod((x + 7) // 8 for x in n)
        return 88 * b + 24 * ((b + 1023) // 1024)
    for n in ((1, 1, 1), (8, 8, 8), (9, 8, 8), (19, 11, 17), (128, 128, 128), (512, 512, 512)):
        assert need(n) == formula(n), n
    assert need((8, 8, 8)) < need((9, 8, 8)) < need((17, 9, 9)) < need((64, 64, 64))
    # 512^3 cells: tens of MB, below 1/8 of the (n + 1)^3 float lattice sdf_sample would need
    assert 10e6 < need((512, 512, 512)) < 4 * 513 ** 3 / 8


def test_obj_round_trip(tmp_path):
    rng = np.random.default_rng(3)
    v = rng.normal(size=(37, 3)).astype(np.float32)
    v[5, 1] = np.nan
    v[6, 0] = np.float32(1e-42)                   # a denormal survives nine digits
    n = rng.normal(size=(37, 3)).astype(np.float32)
    t = rng.integers(0, 37, size=(50, 3)).astype(np.int32)
    for normals in (None, n):
        p = tmp_path / "m.obj"
        meshio.write_obj(p, v, t, normals)
        text = p.read_text().splitlines()
        assert sum(l.startswith("v ") for l in text) == 37
        assert sum(l.startswith("vn ") for l in text) == (37 if normals is not None else 0)
        faces = [l for l in text if l.startswith("f ")]
        assert len(faces) == 50
        first = [int(x.split("/")[0]) for x in faces[0].split()[1:]]
        assert first == (t[0] + 1).tolist()                     # 1-based
        v2, t2, n2 = meshio.read_obj(p)
        assert v2.dtype == np.float32 and t2.dtype == np.int32
        assert np.all((v2.view(np.uint32) == v.view(np.uint32)) | np.isnan(v))
        assert np.isnan(v2[5, 1]) and np.array_equal(t2, t)
        assert (n2 is None) if normals is None else np.array_equal(n2.view(np.uint32), n.view(np.uint32))
    with pytest.raises(ValueError):
        meshio.write_obj(tmp_path / "bad.obj", v, np.array([[0, 1, 37]]))
    meshio.write_obj(tmp_path / "empty.obj", np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int32))
    v0, t0, n0 = meshio.read_obj(tmp_path / "empty.obj")
    assert v0.shape == (0, 3) and t0.shape == (0, 3) and n0 is None
