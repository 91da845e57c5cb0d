"""Binary PLY output of a coloured point cloud: the one format the reconstruction pipeline's fusion step writes and its metrics
step reads (``x y z`` float32, ``red green blue`` uint8, little-endian).  The header is byte for byte what the reference's
``utils/utils_ply.py:write_ply`` produces for float32 xyz and uint8 rgb arrays, so its ``read_ply`` and ``evaluation/metrics.py``
read the file unchanged."""
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
