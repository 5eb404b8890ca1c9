"""Binary PLY files of a textured mesh, numpy only: what `validate_mesh_texture` (exp_runner.py:584-625) exports through
trimesh.  One dialect is written and read back — binary little-endian PLY 1.0 with

    element vertex V:  float x y z [, float nx ny nz] [, uchar red green blue]
    element face T:    property list uchar int vertex_indices   (always 3 indices)

No torch, no GPU: the arrays come from `NeuSRenderer.extract_textured_geometry(...)` (or anywhere else)."""
from __future__ import annotations

import numpy as np

_XYZ, _NRM, _RGB = ("x", "y", "z"), ("nx", "ny", "nz"), ("red", "green", "blue")


def quantize_colors(colors) -> np.ndarray:
    """[V,3] colours as uint8.  Integer input must already be uint8-valued; floating input in [0, 1] is quantised by the
    rule of the library's vertex-colour kernel: rint(255 * clip(x, 0, 1)) in float32."""
    c = np.asarray(colors)
    if c.dtype == np.uint8:
        return c
    if np.issubdtype(c.dtype, np.floating):
        return np.rint(np.clip(c, 0, 1).astype(np.float32) * np.float32(255)).astype(np.uint8)
    if np.issubdtype(c.dtype, np.integer):
        if c.size and (c.min() < 0 or c.max() > 255):
            raise ValueError("write_ply: integer colours must lie in 0..255")
        return c.astype(np.uint8)
    raise ValueError(f"write_ply: colours of dtype {c.dtype}")


def _vertex_dtype(normals: bool, colors: bool) -> np.dtype:
    fields = [(n, "<f4") for n in _XYZ]
    if normals:
        fields += [(n, "<f4") for n in _NRM]
    if colors:
        fields += [(n, "u1") for n in _RGB]
    return np.dtype(fields)


_FACE_DTYPE = np.dtype([("n", "u1"), ("idx", "<i4", (3,))])


def ply_header(n_vertices: int, n_faces: int, normals: bool, colors: bool) -> str:
    lines = ["ply", "format binary_little_endian 1.0", f"element vertex {n_vertices}"]
    lines += [f"property float {n}" for n in _XYZ]
    if normals:
        lines += [f"property float {n}" for n in _NRM]
    if colors:
        lines += [f"property uchar {n}" for n in _RGB]
    lines += [f"element face {n_faces}", "property list uchar int vertex_indices", "end_header"]
    return "\n".join(lines) + "\n"


def write_ply(path, vertices, triangles, normals=None, colors=None, scale_mat=None):
    """Writes the mesh.  vertices [V,3] (stored as float32), triangles [T,3] integer, normals [V,3] (float32) and colors
    [V,3] (uint8 RGB, or floats in [0, 1]: `quantize_colors`) optional.  `scale_mat` [4,4]: the vertices go to world space
    by the reference's expression, `vertices * scale_mat[0, 0] + scale_mat[:3, 3]` (exp_runner.py:573, :594), in float64
    before the conversion to float32; normals are unchanged."""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    t = np.asarray(triangles).reshape(-1, 3)
    if scale_mat is not None:
        s = np.asarray(scale_mat, dtype=np.float64)
        if s.shape != (4, 4):
            raise ValueError(f"write_ply: scale_mat must be [4,4], not {s.shape}")
        v = v * s[0, 0] + s[:3, 3][None]
    V = v.shape[0]
    if t.size and (t.min() < 0 or t.max() >= V):
        raise ValueError("write_ply: a triangle index lies outside the vertex array")
    rec = np.zeros(V, dtype=_vertex_dtype(normals is not None, colors is not None))
    for d, n in enumerate(_XYZ):
        rec[n] = v[:, d].astype(np.float32)
    if normals is not None:
        nr = np.asarray(normals, dtype=np.float32).reshape(-1, 3)
        if nr.shape[0] != V:
            raise ValueError(f"write_ply: {nr.shape[0]} normals for {V} vertices")
        for d, n in enumerate(_NRM):
            rec[n] = nr[:, d]
    if colors is not None:
        c = quantize_colors(colors).reshape(-1, 3)
        if c.shape[0] != V:
            raise ValueError(f"write_ply: {c.shape[0]} colours for {V} vertices")
        for d, n in enumerate(_RGB):
            rec[n] = c[:, d]
    faces = np.zeros(t.shape[0], dtype=_FACE_DTYPE)
    faces["n"] = 3
    faces["idx"] = t.astype(np.int32)
    with open(path, "wb") as f:
        f.write(ply_header(V, t.shape[0], normals is not None, colors is not None).encode("ascii"))
        f.write(rec.tobytes())
        f.write(faces.tobytes())


def read_ply(path) -> dict:
    """Reads a file `write_ply` wrote (that dialect only; anything else raises ValueError).  Returns `vertices` [V,3]
    float32, `triangles` [T,3] int32, `normals` [V,3] float32 or None, `colors` [V,3] uint8 or None."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.find(b"end_header\n")
    if end < 0:
        raise ValueError("read_ply: no end_header")
    lines = data[:end].decode("ascii").split("\n")
    body = data[end + len(b"end_header\n"):]
    if lines[:2] != ["ply", "format binary_little_endian 1.0"] or not lines[2].startswith("element vertex "):
        raise ValueError("read_ply: not a binary little-endian PLY 1.0 of this module's dialect")
    V = int(lines[2].split()[2])
    props, at = [], 3
    while at < len(lines) and lines[at].startswith("property ") and not lines[at].startswith("property list"):
        props.append(tuple(lines[at].split()[1:]))
        at += 1
    want = [("float", n) for n in _XYZ]
    has_n = props[3:6] == [("float", n) for n in _NRM]
    want += [("float", n) for n in _NRM] if has_n else []
    has_c = props[len(want):] == [("uchar", n) for n in _RGB]
    want += [("uchar", n) for n in _RGB] if has_c else []
    rest = [ln for ln in lines[at:] if ln]
    if props != want or len(rest) != 2 or not rest[0].startswith("element face ") \
            or rest[1] != "property list uchar int vertex_indices":
        raise ValueError("read_ply: header is not of this module's dialect")
    T = int(rest[0].split()[2])
    vd = _vertex_dtype(has_n, has_c)
    if len(body) != V * vd.itemsize + T * _FACE_DTYPE.itemsize:
        raise ValueError("read_ply: the body's length does not match the header's counts")
    rec = np.frombuffer(body, dtype=vd, count=V)
    faces = np.frombuffer(body, dtype=_FACE_DTYPE, count=T, offset=V * vd.itemsize)
    if T and not (faces["n"] == 3).all():
        raise ValueError("read_ply: a face that is not a triangle")

    def cols(names, dtype):
        return np.stack([rec[n] for n in names], axis=1).astype(dtype) if V else np.zeros((0, 3), dtype=dtype)

    return {"vertices": cols(_XYZ, np.float32), "triangles": faces["idx"].astype(np.int32).reshape(T, 3),
            "normals": cols(_NRM, np.float32) if has_n else None, "colors": cols(_RGB, np.uint8) if has_c else None}
