"""Binary PLY output of a coloured point cloud: the one format the reconstruction pipeline's fusion step writes and its metrics
step reads (``x y z`` float32, ``red green blue`` uint8, little-endian).  The header is byte for byte what the reference's
``utils/utils_ply.py:write_ply`` produces for float32 xyz and uint8 rgb arrays, so its ``read_ply`` and ``evaluation/metrics.py``
read the file unchanged.  ``read_ply`` is the reader the metrics step uses (any binary property list, like the reference's)."""
from __future__ import annotations

import os

import numpy as np

_VERTEX = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])


def ply_header(n: int) -> bytes:
    lines = ["ply", "format binary_little_endian 1.0", f"element vertex {n}"]
    lines += [f"property float32 {c}" for c in "xyz"] + [f"property uint8 {c}" for c in ("red", "green", "blue")]
    return ("\n".join(lines + ["end_header"]) + "\n").encode("ascii")


def write_point_cloud(path, xyz, rgb) -> None:
    """xyz [M,3] (cast to float32), rgb [M,3] uint8 -> binary little-endian PLY at ``path`` (numpy arrays or tensors)."""
    xyz = np.asarray(getattr(xyz, "cpu", lambda: xyz)(), dtype=np.float32).reshape(-1, 3)
    rgb = np.asarray(getattr(rgb, "cpu", lambda: rgb)())
    if rgb.dtype != np.uint8 or rgb.shape != xyz.shape:
        raise ValueError(f"write_point_cloud: rgb must be uint8 {xyz.shape}, got {rgb.dtype} {rgb.shape}")
    data = np.empty(xyz.shape[0], dtype=_VERTEX)
    for k, c in enumerate("xyz"):
        data[c] = xyz[:, k]
    for k, c in enumerate(("red", "green", "blue")):
        data[c] = rgb[:, k]
    tmp = f"{path}.part"
    with open(tmp, "wb") as fh:
        fh.write(ply_header(xyz.shape[0]))
        fh.write(data.tobytes())
    os.replace(tmp, path)


_COLMAP_VERTEX = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"), ("red", "u1"),
                           ("green", "u1"), ("blue", "u1")])


def colmap_ply_header(n: int) -> bytes:
    """The header COLMAP's stereo fusion writes for a binary fused point cloud (``float x y z nx ny nz``, ``uchar red green blue``)."""
    lines = ["ply", "format binary_little_endian 1.0", f"element vertex {n}"]
    lines += [f"property float {c}" for c in ("x", "y", "z", "nx", "ny", "nz")] + [f"property uchar {c}" for c in ("red", "green", "blue")]
    return ("\n".join(lines + ["end_header"]) + "\n").encode("ascii")


def write_colmap_point_cloud(path, xyz, normal, rgb) -> None:
    """xyz, normal [M,3] (cast to float32), rgb [M,3] uint8 -> binary little-endian PLY in COLMAP's fused layout at ``path``."""
    xyz = np.asarray(getattr(xyz, "cpu", lambda: xyz)(), dtype=np.float32).reshape(-1, 3)
    normal = np.asarray(getattr(normal, "cpu", lambda: normal)(), dtype=np.float32).reshape(-1, 3)
    rgb = np.asarray(getattr(rgb, "cpu", lambda: rgb)())
    if rgb.dtype != np.uint8 or rgb.shape != xyz.shape or normal.shape != xyz.shape:
        raise ValueError(f"write_colmap_point_cloud: normal float [M,3] and rgb uint8 [M,3] expected for {xyz.shape[0]} points")
    data = np.empty(xyz.shape[0], dtype=_COLMAP_VERTEX)
    for k, c in enumerate("xyz"):
        data[c] = xyz[:, k]
        data["n" + c] = normal[:, k]
    for k, c in enumerate(("red", "green", "blue")):
        data[c] = rgb[:, k]
    tmp = f"{path}.part"
    with open(tmp, "wb") as fh:
        fh.write(colmap_ply_header(xyz.shape[0]))
        fh.write(data.tobytes())
    os.replace(tmp, path)


# the reference's ply_dtypes (utils/utils_ply.py; its later "uchar" entry wins)
PLY_DTYPES = {b"int8": "i1", b"char": "i1", b"uint8": "u1", b"uchar": "u1", b"int16": "i2", b"short": "i2", b"uint16": "u2",
              b"ushort": "u2", b"int32": "i4", b"int": "i4", b"uint32": "u4", b"uint": "u4", b"float32": "f4", b"float": "f4",
              b"float64": "f8", b"double": "f8"}
_PLY_FORMATS = {"binary_big_endian": ">", "binary_little_endian": "<"}


def read_ply(path) -> np.ndarray:
    """Structured array of a binary PLY file with one element list (what the reference's ``read_ply`` returns).  The point
    cloud's coordinates feed float32 kernels, so a file whose ``x``, ``y`` or ``z`` is float64 is rejected rather than rounded."""
    with open(path, "rb") as fh:
        if b"ply" not in fh.readline():
            raise ValueError(f"{path}: not a PLY file")
        fmt = fh.readline().split()[1].decode()
        if fmt not in _PLY_FORMATS:
            raise ValueError(f"{path}: PLY format {fmt!r} is not binary")
        ext = _PLY_FORMATS[fmt]
        props, n, line = [], None, b""
        while b"end_header" not in line:
            line = fh.readline()
            if line == b"":
                raise ValueError(f"{path}: truncated PLY header")
            if b"element" in line:
                n = int(line.split()[2])
            elif b"property" in line:
                tok = line.split()
                if tok[1] not in PLY_DTYPES:
                    raise ValueError(f"{path}: unsupported PLY property type {tok[1].decode()!r}")
                props.append((tok[2].decode(), ext + PLY_DTYPES[tok[1]]))
        wide = [name for name, dt in props if name in ("x", "y", "z") and dt.endswith("f8")]
        if wide:
            raise ValueError(f"{path}: coordinates {', '.join(wide)} are float64; the metrics run on float32 points and will not "
                             f"round them silently")
        return np.fromfile(fh, dtype=props, count=n)


# ---- triangle meshes (evaluation/tsdf_fusion.py) ----------------------------------------------------------------------------------
_FACE = np.dtype([("n", "u1"), ("v", "<i4", (3,))])


_VERTEX_NORMAL = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"), ("red", "u1"),
                           ("green", "u1"), ("blue", "u1")])


def mesh_ply_header(n_vertices: int, n_faces: int, normals: bool = False) -> bytes:
    lines = ["ply", "format binary_little_endian 1.0", f"element vertex {n_vertices}"]
    lines += [f"property float32 {c}" for c in (("x", "y", "z", "nx", "ny", "nz") if normals else "xyz")]
    lines += [f"property uint8 {c}" for c in ("red", "green", "blue")]
    lines += [f"element face {n_faces}", "property list uchar int vertex_indices"]
    return ("\n".join(lines + ["end_header"]) + "\n").encode("ascii")


def write_mesh(path, xyz, rgb, faces, normals=None) -> None:
    """xyz [V,3] (cast to float32), rgb [V,3] uint8, faces [F,3] integer indices into the vertices -> binary little-endian PLY at
    ``path`` with ``element face`` / ``property list uchar int vertex_indices`` (numpy arrays or tensors).  With ``normals`` [V,3]
    (cast to float32) the vertices also carry ``property float32 nx / ny / nz`` after ``z``; without, the file is what it always was."""
    xyz = np.asarray(getattr(xyz, "cpu", lambda: xyz)(), dtype=np.float32).reshape(-1, 3)
    if normals is not None:
        normals = np.asarray(getattr(normals, "cpu", lambda: normals)(), dtype=np.float32)
        if normals.shape != xyz.shape:
            raise ValueError(f"write_mesh: normals must be float {xyz.shape}, got {normals.shape}")
    rgb = np.asarray(getattr(rgb, "cpu", lambda: rgb)())
    faces = np.asarray(getattr(faces, "cpu", lambda: faces)())
    if rgb.dtype != np.uint8 or rgb.shape != xyz.shape:
        raise ValueError(f"write_mesh: rgb must be uint8 {xyz.shape}, got {rgb.dtype} {rgb.shape}")
    if faces.dtype.kind not in "iu" or faces.ndim != 2 or faces.shape[1] != 3:
        raise ValueError(f"write_mesh: faces must be integer [F,3], got {faces.dtype} {faces.shape}")
    if faces.size and (int(faces.min()) < 0 or int(faces.max()) >= xyz.shape[0]):
        raise ValueError(f"write_mesh: face indices must lie in [0, {xyz.shape[0]})")
    vdata = np.empty(xyz.shape[0], dtype=_VERTEX if normals is None else _VERTEX_NORMAL)
    for k, c in enumerate("xyz"):
        vdata[c] = xyz[:, k]
        if normals is not None:
            vdata["n" + c] = normals[:, k]
    for k, c in enumerate(("red", "green", "blue")):
        vdata[c] = rgb[:, k]
    fdata = np.empty(faces.shape[0], dtype=_FACE)
    fdata["n"] = 3
    fdata["v"] = faces
    tmp = f"{path}.part"
    with open(tmp, "wb") as fh:
        fh.write(mesh_ply_header(xyz.shape[0], faces.shape[0], normals is not None))
        fh.write(vdata.tobytes())
        fh.write(fdata.tobytes())
    os.replace(tmp, path)


def read_mesh(path):
    """(xyz float32 [V,3], rgb uint8 [V,3], faces int32 [F,3]) of a binary little-endian PLY triangle mesh as ``write_mesh`` writes
    it: vertex properties by name (x, y, z float32 and red, green, blue uint8 must be among them), faces as a uchar-counted list of
    int / uint indices, every face a triangle."""
    return read_mesh_normals(path)[:3]


def read_mesh_normals(path):
    """``read_mesh`` plus the vertex normals: (xyz, rgb, faces, normals float32 [V,3]), normals None for a file without the float32
    properties nx, ny, nz."""
    with open(path, "rb") as fh:
        if b"ply" not in fh.readline():
            raise ValueError(f"{path}: not a PLY file")
        fmt = fh.readline().split()[1].decode()
        if fmt != "binary_little_endian":
            raise ValueError(f"{path}: PLY format {fmt!r} is not binary_little_endian")
        counts, props, index_type, element, line = {}, [], None, None, b""
        while b"end_header" not in line:
            line = fh.readline()
            if line == b"":
                raise ValueError(f"{path}: truncated PLY header")
            tok = line.split()
            if tok[:1] == [b"element"]:
                element = tok[1].decode()
                counts[element] = int(tok[2])
            elif tok[:1] == [b"property"]:
                if element == "vertex":
                    if tok[1] not in PLY_DTYPES:
                        raise ValueError(f"{path}: unsupported PLY property type {tok[1].decode()!r}")
                    props.append((tok[2].decode(), "<" + PLY_DTYPES[tok[1]]))
                elif element == "face":
                    if tok[1] != b"list" or PLY_DTYPES.get(tok[2]) != "u1" or PLY_DTYPES.get(tok[3]) not in ("i4", "u4"):
                        raise ValueError(f"{path}: faces must be `property list uchar int vertex_indices`")
                    index_type = "<" + PLY_DTYPES[tok[3]]
        if "vertex" not in counts or "face" not in counts or index_type is None or list(counts) != ["vertex", "face"]:
            raise ValueError(f"{path}: a mesh needs `element vertex` followed by `element face`")
        vdata = np.fromfile(fh, dtype=props, count=counts["vertex"])
        fdata = np.fromfile(fh, dtype=np.dtype([("n", "u1"), ("v", index_type, (3,))]), count=counts["face"])
    if vdata.shape[0] != counts["vertex"] or fdata.shape[0] != counts["face"]:
        raise ValueError(f"{path}: truncated PLY data")
    if fdata.size and (fdata["n"] != 3).any():
        raise ValueError(f"{path}: every face must be a triangle")
    for c in ("x", "y", "z"):
        if vdata.dtype[c] != np.dtype("<f4"):
            raise ValueError(f"{path}: coordinate {c} must be float32")
    xyz = np.stack([vdata[c] for c in "xyz"], axis=-1).astype(np.float32).reshape(-1, 3)
    rgb = np.stack([vdata[c] for c in ("red", "green", "blue")], axis=-1).astype(np.uint8).reshape(-1, 3)
    normals = None
    if all(c in vdata.dtype.names and vdata.dtype[c] == np.dtype("<f4") for c in ("nx", "ny", "nz")):
        normals = np.stack([vdata[c] for c in ("nx", "ny", "nz")], axis=-1).astype(np.float32).reshape(-1, 3)
    return xyz, rgb, fdata["v"].astype(np.int32).reshape(-1, 3), normals
