"""Vertex colours in sdf3d_amd.meshio (CPU): the binary PLY round trip, the
byte a colour component becomes (the RGBA8 rule of include/sdf_abi.h, NaN and
out-of-range values included), and an OBJ without colours byte for byte what
the writer gave before it knew of them."""
import numpy as np
import pytest

from sdf3d_amd import meshio

f32 = np.float32


def mesh(nv=7):
    rng = np.random.default_rng(5)
    v = rng.standard_normal((nv, 3)).astype(f32)
    v[1] = (np.nan, np.inf, -0.0)
    n = rng.standard_normal((nv, 3)).astype(f32)
    t = np.array([[0, 1, 2], [2, 3, 4], [4, 5, 6], [6, 0, 3]], dtype=np.int32)
    c = rng.random((nv, 4)).astype(f32)
    return v, t, n, c


def same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("normals,colors", [(False, False), (True, False), (False, True),
                                            (True, True)])
def test_ply_round_trip(tmp_path, normals, colors):
    v, t, n, c = mesh()
    p = tmp_path / "m.ply"
    meshio.write_ply(p, v, t, n if normals else None, c if colors else None)
    head = p.read_bytes().split(b"end_header\n")[0].decode("ascii").splitlines()
    assert head[:2] == ["ply", "format binary_little_endian 1.0"]
    assert ("property float nx" in head) == normals
    assert ("property uchar red" in head) == colors
    V, T, N, Cb = meshio.read_ply(p)
    assert same(V, v) and np.array_equal(T, t) and T.dtype == np.int32
    assert (N is None) != normals and (Cb is None) != colors
    if normals:
        assert same(N, n)
    if colors:
        assert Cb.dtype == np.uint8 and np.array_equal(Cb, meshio.colors_u8(c[:, :3]))
        # bytes in, the same bytes out
        meshio.write_ply(p, v, t, None, Cb)
        assert np.array_equal(meshio.read_ply(p)[3], Cb)


def test_ply_length_is_header_plus_records(tmp_path):
    v, t, n, c = mesh()
    p = tmp_path / "m.ply"
    meshio.write_ply(p, v, t, n, c)
    data = p.read_bytes()
    body = len(data) - (data.index(b"end_header\n") + 11)
    assert body == len(v) * (12 + 12 + 3) + len(t) * 13
    p.write_bytes(data[:-1])
    with pytest.raises(ValueError):
        meshio.read_ply(p)


def test_empty_mesh(tmp_path):
    p = tmp_path / "e.ply"
    meshio.write_ply(p, np.zeros((0, 3), f32), np.zeros((0, 3), np.int32), None,
                     np.zeros((0, 3), f32))
    V, T, N, Cb = meshio.read_ply(p)
    assert V.shape == (0, 3) and T.shape == (0, 3) and N is None and Cb.shape == (0, 3)


def test_u8_rule():
    """u8 = trunc(min(max(c, 0), 1) * 255 + 0.5) in fp32, NaN -> 0."""
    c = np.array([0.0, 1.0, 0.5, -0.0, -1.0, 2.0, np.nan, np.inf, -np.inf, 1e-9,
                  0.5 / 255, np.nextafter(f32(0.5 / 255), f32(0)), 254.5 / 255, 0.999, 1 / 3],
                 dtype=f32)
    want = [0, 255, 128, 0, 0, 255, 0, 255, 0, 0]
    got = meshio.colors_u8(c)
    assert got.dtype == np.uint8 and list(got[:10]) == want
    # every fp32 step of the rule, restated per element
    for x, g in zip(c, got):
        y = f32(0) if np.isnan(x) else min(max(x, f32(0)), f32(1))
        assert int(g) == int(np.trunc(f32(f32(y * f32(255)) + f32(0.5)))), x
    # all 256 bytes come back from their own value / 255
    ramp = (np.arange(256, dtype=f32) / f32(255)).astype(f32)
    assert np.array_equal(meshio.colors_u8(ramp), np.arange(256, dtype=np.uint8))


def test_colour_count_must_match(tmp_path):
    v, t, n, c = mesh()
    with pytest.raises(ValueError):
        meshio.write_ply(tmp_path / "x.ply", v, t, None, c[:-1])
    with pytest.raises(ValueError):
        meshio.write_obj(tmp_path / "x.obj", v, t, None, c[:, :2])


def old_write_obj(path, verts, tris, normals=None):
    """The writer as it was before `colors=`, kept here as the yardstick."""
    v = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
    t = np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    n = None if normals is None else np.asarray(normals, dtype=np.float32).reshape(-1, 3)
    lines = [f"# {len(v)} vertices, {len(t)} triangles"]
    lines += ["v %.9g %.9g %.9g" % tuple(float(x) for x in p) for p in v]
    if n is not None:
        lines += ["vn %.9g %.9g %.9g" % tuple(float(x) for x in p) for p in n]
        lines += ["f %d//%d %d//%d %d//%d" % (a, a, b, b, c, c) for a, b, c in (t + 1).tolist()]
    else:
        lines += ["f %d %d %d" % (a, b, c) for a, b, c in (t + 1).tolist()]
    path.write_text("\n".join(lines) + "\n")


@pytest.mark.parametrize("normals", [False, True])
def test_obj_without_colours_is_byte_identical(tmp_path, normals):
    v, t, n, _ = mesh()
    a, b = tmp_path / "a.obj", tmp_path / "b.obj"
    meshio.write_obj(a, v, t, n if normals else None)
    old_write_obj(b, v, t, n if normals else None)
    assert a.read_bytes() == b.read_bytes()


def test_obj_with_colours(tmp_path):
    v, t, n, c = mesh()
    p = tmp_path / "c.obj"
    meshio.write_obj(p, v, t, n, colors=c)
    rows = [l.split() for l in p.read_text().splitlines() if l.startswith("v ")]
    assert len(rows) == len(v) and all(len(r) == 7 for r in rows)
    got = np.array([[float(x) for x in r[4:7]] for r in rows], dtype=f32)
    assert same(got, np.ascontiguousarray(c[:, :3]))
    # positions, normals and faces read back as before
    V, T, N = meshio.read_obj(p)
    assert same(V, v) and np.array_equal(T, t) and same(N, n)
