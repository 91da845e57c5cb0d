"""COLMAP's dense ``Mat`` files (``src/mvs/mat.h``): an ASCII header ``W&H&C&`` followed by W x H x C little-endian fp32 in
column-major (x fastest, channel slowest) order.  Vectorised ``read_array`` / ``write_array`` with the reference's interface
(``utils/colmap_utils.py``); the reference packs the floats through ``struct`` one by one."""
from __future__ import annotations

import numpy as np


def read_array(path) -> np.ndarray:
    """-> fp32 [H,W] (one channel) or [H,W,C]."""
    with open(path, "rb") as fid:
        data = fid.read()
    pos = -1
    for _ in range(3):
        pos = data.index(b"&", pos + 1)
    width, height, channels = (int(x) for x in data[:pos].split(b"&"))
    arr = np.frombuffer(data, dtype="<f4", offset=pos + 1, count=width * height * channels)
    arr = arr.reshape((channels, height, width)).transpose(1, 2, 0)
    return np.ascontiguousarray(arr.squeeze())


def write_array(array: np.ndarray, path) -> None:
    """fp32 [H,W] or [H,W,C] -> a Mat file, byte for byte what the reference's writer produces."""
    if array.dtype != np.float32:
        raise ValueError(f"write_array: float32 expected, got {array.dtype}")
    if array.ndim == 2:
        height, width = array.shape
        channels = 1
        planes = array[None]
    elif array.ndim == 3:
        height, width, channels = array.shape
        planes = array.transpose(2, 0, 1)
    else:
        raise ValueError(f"write_array: [H,W] or [H,W,C] expected, got {array.shape}")
    with open(path, "wb") as fid:
        fid.write(f"{width}&{height}&{channels}&".encode("ascii"))
        fid.write(np.ascontiguousarray(planes, dtype="<f4").tobytes())
