"""mesh_io.write_ply / read_ply (numpy only, no GPU): the binary PLY dialect of the textured-mesh export."""
import numpy as np
import pytest

from rnb_neus_fork_amd import mesh_io


def _mesh(V=37, T=61, seed=0):
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((V, 3))
    n = rng.standard_normal((V, 3)).astype(np.float32)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    c = rng.integers(0, 256, size=(V, 3), dtype=np.uint8)
    t = rng.integers(0, V, size=(T, 3)).astype(np.int32)
    return v, t, n, c


@pytest.mark.parametrize("with_normals,with_colors", [(True, True), (True, False), (False, True), (False, False)])
def test_round_trip_is_bit_equal(tmp_path, with_normals, with_colors):
    v, t, n, c = _mesh()
    path = tmp_path / "m.ply"
    mesh_io.write_ply(path, v, t, normals=n if with_normals else None, colors=c if with_colors else None)
    m = mesh_io.read_ply(path)
    assert m["vertices"].dtype == np.float32 and np.array_equal(m["vertices"], v.astype(np.float32))
    assert m["triangles"].dtype == np.int32 and np.array_equal(m["triangles"], t)
    if with_normals:
        assert m["normals"].dtype == np.float32 and np.array_equal(m["normals"], n)
    else:
        assert m["normals"] is None
    if with_colors:
        assert m["colors"].dtype == np.uint8 and np.array_equal(m["colors"], c)
    else:
        assert m["colors"] is None


def test_header_and_layout(tmp_path):
    v, t, n, c = _mesh(V=5, T=2)
    path = tmp_path / "m.ply"
    mesh_io.write_ply(path, v, t, normals=n, colors=c)
    data = path.read_bytes()
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex 5\n"
              "property float x\nproperty float y\nproperty float z\n"
              "property float nx\nproperty float ny\nproperty float nz\n"
              "property uchar red\nproperty uchar green\nproperty uchar blue\n"
              "element face 2\nproperty list uchar int vertex_indices\nend_header\n")
    assert data.startswith(header.encode("ascii"))
    body = data[len(header):]
    assert len(body) == 5 * (6 * 4 + 3) + 2 * (1 + 3 * 4)
    # the first vertex record and the first face, byte for byte
    first = v[0].astype("<f4").tobytes() + n[0].astype("<f4").tobytes() + c[0].tobytes()
    assert body[:27] == first
    assert body[5 * 27:5 * 27 + 13] == b"\x03" + t[0].astype("<i4").tobytes()
    # without the optional properties the header has neither
    mesh_io.write_ply(path, v, t)
    text = path.read_bytes().split(b"end_header\n")[0].decode()
    assert "nx" not in text and "red" not in text and "element vertex 5" in text


def test_scale_mat_moves_vertices_and_leaves_normals(tmp_path):
    v, t, n, c = _mesh()
    s = np.eye(4)
    s[0, 0] = s[1, 1] = s[2, 2] = 2.75
    s[:3, 3] = [0.5, -1.25, 3.0]
    path = tmp_path / "m.ply"
    mesh_io.write_ply(path, v, t, normals=n, colors=c, scale_mat=s)
    m = mesh_io.read_ply(path)
    assert np.array_equal(m["vertices"], (v * s[0, 0] + s[:3, 3][None]).astype(np.float32))
    assert np.array_equal(m["normals"], n) and np.array_equal(m["triangles"], t)
    with pytest.raises(ValueError, match="scale_mat"):
        mesh_io.write_ply(path, v, t, scale_mat=np.eye(3))


def test_empty_mesh(tmp_path):
    path = tmp_path / "e.ply"
    mesh_io.write_ply(path, np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int32), normals=np.zeros((0, 3), dtype=np.float32),
                      colors=np.zeros((0, 3), dtype=np.uint8))
    m = mesh_io.read_ply(path)
    assert m["vertices"].shape == (0, 3) and m["triangles"].shape == (0, 3)
    assert m["normals"].shape == (0, 3) and m["colors"].shape == (0, 3)
    assert m["triangles"].dtype == np.int32 and m["colors"].dtype == np.uint8


def test_float_colours_are_quantised_by_the_kernel_rule(tmp_path):
    rng = np.random.default_rng(3)
    x = rng.uniform(-0.2, 1.2, size=(400, 3))
    x[:6, 0] = [0.0, 1.0, 0.5 / 255, 1.5 / 255, 2.5 / 255, 254.5 / 255]      # ends of the range and rounding ties
    v = rng.standard_normal((400, 3))
    want = np.rint(np.clip(x, 0, 1).astype(np.float32) * np.float32(255)).astype(np.uint8)
    path = tmp_path / "c.ply"
    for colours in (x, x.astype(np.float32)):
        mesh_io.write_ply(path, v, np.zeros((0, 3), dtype=np.int32), colors=colours)
        got = mesh_io.read_ply(path)["colors"]
        ref = np.rint(np.clip(colours, 0, 1).astype(np.float32) * np.float32(255)).astype(np.uint8)
        assert np.array_equal(got, ref)
    assert np.array_equal(got, want)   # (fp32 input last: the same bits as converting the fp64 input)
    assert want.min() == 0 and want.max() == 255


def test_refusals(tmp_path):
    v, t, n, c = _mesh(V=4, T=2)
    path = tmp_path / "m.ply"
    with pytest.raises(ValueError, match="triangle index"):
        mesh_io.write_ply(path, v, np.array([[0, 1, 4]]))
    with pytest.raises(ValueError, match="normals"):
        mesh_io.write_ply(path, v, t, normals=n[:3])
    path.write_bytes(b"ply\nformat ascii 1.0\nelement vertex 0\nend_header\n")
    with pytest.raises(ValueError):
        mesh_io.read_ply(path)
