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
