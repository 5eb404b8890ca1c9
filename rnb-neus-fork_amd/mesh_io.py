"""Binary PLY files of a textured mesh, numpy only: what `validate_mesh_texture` (exp_runner.py:584-625) exports through
trimesh.  One dialect is written and read back — binary little-endian PLY 1.0 with

    element vertex V:  float x y z [, float nx ny nz] [, uchar red green blue]
    element face T:    property list uchar int vertex_indices   (always 3 indices)

No torch, no GPU: the arrays come from `NeuSRenderer.extract_textured_geometry(...)` (or anywhere else).

A UV-mapped mesh with baked textures (`NeuSRenderer.bake_textures`) goes out as Wavefront OBJ + MTL (`write_obj` /
`read_obj`: one `vt` per triangle corner) and 8-bit PNG images (`write_png` / `read_png`, standard library only)."""
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


# ---- Wavefront OBJ / MTL of a UV-mapped mesh, and 8-bit PNG images: what a baked mesh (`NeuSRenderer.bake_textures`) is
# exported as.  Text and zlib / struct from the standard library; no image library is needed.

_MATERIAL_NAME = "baked"


def write_obj(path, vertices, triangles, uv, normals=None, scale_mat=None, material=None):
    """Writes `v` lines (float64, 17 significant digits: they read back bit for bit), one `vt` per triangle corner from
    uv [T,3,2], optional `vn` per vertex from normals [V,3] (float32, 9 digits) and faces `f a/ta` or `f a/ta/na`, 1-based.
    `scale_mat` as in `write_ply`.  `material`: a dict with `albedo` and / or `normal` (image file names, as they should
    appear in the file) — a `<path stem>.mtl` is written beside the OBJ (newmtl baked, map_Kd = albedo, norm = normal) and
    the OBJ names it (mtllib / usemtl)."""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    t = np.asarray(triangles).reshape(-1, 3).astype(np.int64)
    tc = np.asarray(uv, dtype=np.float64)
    if tc.shape != (t.shape[0], 3, 2):
        raise ValueError(f"write_obj: uv must be [T,3,2] with T = {t.shape[0]}, not {tc.shape}")
    if scale_mat is not None:
        s = np.asarray(scale_mat, dtype=np.float64)
        if s.shape != (4, 4):
            raise ValueError(f"write_obj: scale_mat must be [4,4], not {s.shape}")
        v = v * s[0, 0] + s[:3, 3][None]
    V = v.shape[0]
    if t.size and (t.min() < 0 or t.max() >= V):
        raise ValueError("write_obj: a triangle index lies outside the vertex array")
    nr = None
    if normals is not None:
        nr = np.asarray(normals, dtype=np.float32).reshape(-1, 3)
        if nr.shape[0] != V:
            raise ValueError(f"write_obj: {nr.shape[0]} normals for {V} vertices")
    path = str(path)
    lines = []
    if material is not None:
        if not isinstance(material, dict) or not set(material) <= {"albedo", "normal"} or not material:
            raise ValueError("write_obj: material must be a dict with `albedo` and / or `normal` image file names")
        stem = path[:-4] if path.lower().endswith(".obj") else path
        with open(stem + ".mtl", "w") as f:
            f.write(f"newmtl {_MATERIAL_NAME}\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\n")
            if "albedo" in material:
                f.write(f"map_Kd {material['albedo']}\n")
            if "normal" in material:
                f.write(f"norm {material['normal']}\n")
        lines += [f"mtllib {stem.replace(chr(92), '/').rsplit('/', 1)[-1]}.mtl", f"usemtl {_MATERIAL_NAME}"]
    lines += ["v %.17g %.17g %.17g" % tuple(p) for p in v.tolist()]
    lines += ["vt %.17g %.17g" % tuple(p) for p in tc.reshape(-1, 2).tolist()]
    if nr is not None:
        lines += ["vn %.9g %.9g %.9g" % tuple(p) for p in nr.astype(np.float64).tolist()]
    for k, (a, b, c) in enumerate((t + 1).tolist()):
        if nr is None:
            lines.append(f"f {a}/{3 * k + 1} {b}/{3 * k + 2} {c}/{3 * k + 3}")
        else:
            lines.append(f"f {a}/{3 * k + 1}/{a} {b}/{3 * k + 2}/{b} {c}/{3 * k + 3}/{c}")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def read_obj(path) -> dict:
    """Reads a file `write_obj` wrote (that dialect only).  Returns `vertices` [V,3] float64, `triangles` [T,3] int32,
    `uv` [T,3,2] float64, `normals` [V,3] float32 or None and `material`: None, or the dict given to `write_obj` (read
    from the MTL file beside the OBJ)."""
    import os
    v, vt, vn, faces, mtllib = [], [], [], [], None
    with open(path) as f:
        for ln in f:
            p = ln.split()
            if not p or p[0] == "usemtl":
                continue
            if p[0] == "v":
                v.append([float(x) for x in p[1:4]])
            elif p[0] == "vt":
                vt.append([float(x) for x in p[1:3]])
            elif p[0] == "vn":
                vn.append([float(x) for x in p[1:4]])
            elif p[0] == "f" and len(p) == 4:
                faces.append([[int(i) for i in c.split("/")] for c in p[1:]])
            elif p[0] == "mtllib":
                mtllib = ln.split(None, 1)[1].strip()
            else:
                raise ValueError(f"read_obj: a line that is not of this module's dialect: {ln.strip()!r}")
    V, T = len(v), len(faces)
    fa = np.asarray(faces, dtype=np.int64).reshape(T, 3, -1) if T else np.zeros((0, 3, 3 if vn else 2), dtype=np.int64)
    if fa.shape[2] != (3 if vn else 2) or len(vt) != 3 * T or (vn and len(vn) != V):
        raise ValueError("read_obj: faces, texture coordinates and normals do not fit this module's dialect")
    if T and (fa[..., 0].min() < 1 or fa[..., 0].max() > V or not np.array_equal(fa[..., 1].reshape(-1), np.arange(1, 3 * T + 1))
              or (vn and not np.array_equal(fa[..., 2], fa[..., 0]))):
        raise ValueError("read_obj: face indices do not fit this module's dialect")
    material = None
    if mtllib is not None:
        material = {}
        with open(os.path.join(os.path.dirname(str(path)), mtllib)) as f:
            for ln in f:
                p = ln.split(None, 1)
                if len(p) == 2 and p[0] in ("map_Kd", "norm"):
                    material["albedo" if p[0] == "map_Kd" else "normal"] = p[1].strip()
    return {"vertices": np.asarray(v, dtype=np.float64).reshape(V, 3), "triangles": (fa[..., 0] - 1).astype(np.int32),
            "uv": np.asarray(vt, dtype=np.float64).reshape(T, 3, 2),
            "normals": np.asarray(vn, dtype=np.float32).reshape(V, 3) if vn else None, "material": material}


_PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"


def _png_chunk(kind: bytes, data: bytes) -> bytes:
    import struct
    import zlib
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def write_png(path, image):
    """Writes image [H,W,3] or [H,W,4] uint8 (row 0 on top) as an 8-bit RGB / RGBA PNG, non-interlaced, filter 0 on every
    row.  H, W >= 1."""
    import struct
    import zlib
    img = np.asarray(image)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] not in (3, 4) or img.shape[0] < 1 or img.shape[1] < 1:
        raise ValueError(f"write_png: image must be uint8 [H,W,3] or [H,W,4] with H, W >= 1, not {img.dtype} {img.shape}")
    H, W, Cn = img.shape
    raw = np.zeros((H, 1 + W * Cn), dtype=np.uint8)
    raw[:, 1:] = img.reshape(H, W * Cn)
    ihdr = struct.pack(">IIBBBBB", W, H, 8, 2 if Cn == 3 else 6, 0, 0, 0)
    with open(path, "wb") as f:
        f.write(_PNG_SIGNATURE + _png_chunk(b"IHDR", ihdr) + _png_chunk(b"IDAT", zlib.compress(raw.tobytes()))
                + _png_chunk(b"IEND", b""))


def read_png(path) -> np.ndarray:
    """Reads an 8-bit RGB or RGBA, non-interlaced PNG (all five row filters; ancillary chunks are skipped, checksums are
    verified): [H,W,3] or [H,W,4] uint8.  Anything else raises ValueError."""
    import struct
    import zlib
    with open(path, "rb") as f:
        data = f.read()
    if data[:8] != _PNG_SIGNATURE:
        raise ValueError("read_png: not a PNG file")
    at, ihdr, idat, ended = 8, None, [], False
    while at + 12 <= len(data) and not ended:
        n, kind = struct.unpack(">I", data[at:at + 4])[0], data[at + 4:at + 8]
        body = data[at + 8:at + 8 + n]
        if len(body) != n or struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0] != (zlib.crc32(kind + body) & 0xFFFFFFFF):
            raise ValueError("read_png: a truncated chunk or a wrong checksum")
        if kind == b"IHDR":
            ihdr = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat.append(body)
        elif kind == b"IEND":
            ended = True
        elif not (kind[0] & 0x20):
            raise ValueError(f"read_png: critical chunk {kind!r} is not supported")
        at += 12 + n
    if ihdr is None or not ended:
        raise ValueError("read_png: no IHDR or no IEND")
    W, H, depth, ctype, comp, filt, interlace = ihdr
    if depth != 8 or ctype not in (2, 6) or comp != 0 or filt != 0 or interlace != 0 or W < 1 or H < 1:
        raise ValueError("read_png: only 8-bit RGB / RGBA, non-interlaced images are supported")
    bpp = 3 if ctype == 2 else 4
    stride = W * bpp
    raw = np.frombuffer(zlib.decompress(b"".join(idat)), dtype=np.uint8)
    if raw.size != H * (stride + 1):
        raise ValueError("read_png: the image data's length does not match the header")
    raw = raw.reshape(H, stride + 1)
    out = np.zeros((H, stride), dtype=np.uint8)
    prev = np.zeros(stride, dtype=np.int64)
    for y in range(H):
        ft, line = int(raw[y, 0]), raw[y, 1:].astype(np.int64)
        if ft == 0:
            cur = line
        elif ft == 1:      # Sub: a running sum per channel
            cur = np.cumsum(line.reshape(W, bpp), axis=0).reshape(-1) & 255
        elif ft == 2:      # Up
            cur = (line + prev) & 255
        elif ft in (3, 4):  # Average / Paeth: each byte needs its left neighbour's result
            cur = np.zeros(stride, dtype=np.int64)
            ln, pv = line.tolist(), prev.tolist()
            res = [0] * stride
            for i in range(stride):
                a = res[i - bpp] if i >= bpp else 0
                b = pv[i]
                if ft == 3:
                    pred = (a + b) >> 1
                else:
                    c = pv[i - bpp] if i >= bpp else 0
                    p = a + b - c
                    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                    pred = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
                res[i] = (ln[i] + pred) & 255
            cur = np.asarray(res, dtype=np.int64)
        else:
            raise ValueError(f"read_png: unknown row filter {ft}")
        out[y] = cur.astype(np.uint8)
        prev = cur
    return out.reshape(H, W, bpp)
