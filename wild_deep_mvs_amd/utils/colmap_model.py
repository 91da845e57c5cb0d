"""Minimal reader of COLMAP's binary sparse model: ``cameras.bin`` (intrinsics), ``images.bin`` (poses, image names and the 3-D
point each keypoint observes) and ``points3D.bin`` (point tracks), written from COLMAP's documented layout (little-endian):

    cameras.bin   uint64 n; per camera: int32 camera_id, int32 model_id, uint64 width, uint64 height, then the model's
                  parameters as doubles (SIMPLE_PINHOLE f cx cy; PINHOLE fx fy cx cy; ... the table of COLMAP's camera models)
    images.bin    uint64 n; per image: uint32 image_id, double qvec[4], double tvec[3], uint32 camera_id, name (NUL-terminated),
                  uint64 n_points2D, then n_points2D x (double x, double y, int64 point3D_id; -1 when unmatched)
    points3D.bin  uint64 n; per point: uint64 point3D_id, double xyz[3], uint8 rgb[3], double error, uint64 track_length,
                  then track_length x (uint32 image_id, uint32 point2D_idx)

The fusion step needs only which images see which points (``shared_point_counts``), to order COLMAP's overlapping images.
Scene set-up (``utils/colmap_utils.py``) reads all three files.
Without a sparse model the same lists come from the depth maps (``overlap_from_covisibility`` over ``ops.view_covisibility``)."""
from __future__ import annotations

import struct
from collections import namedtuple
from pathlib import Path

import numpy as np

Camera = namedtuple("Camera", ["id", "model", "width", "height", "params"])
Image = namedtuple("Image", ["id", "qvec", "tvec", "camera_id", "name", "xys", "point3D_ids"])
Point3D = namedtuple("Point3D", ["id", "xyz", "rgb", "error", "image_ids", "point2D_idxs"])


def _read(fh, fmt):
    size = struct.calcsize("<" + fmt)
    buf = fh.read(size)
    if len(buf) != size:
        raise ValueError(f"{fh.name}: truncated COLMAP model file")
    return struct.unpack("<" + fmt, buf)


# COLMAP's camera models: model_id -> (name, number of parameters)
CAMERA_MODELS = {0: ("SIMPLE_PINHOLE", 3), 1: ("PINHOLE", 4), 2: ("SIMPLE_RADIAL", 4), 3: ("RADIAL", 5), 4: ("OPENCV", 8),
                 5: ("OPENCV_FISHEYE", 8), 6: ("FULL_OPENCV", 12), 7: ("FOV", 5), 8: ("SIMPLE_RADIAL_FISHEYE", 4),
                 9: ("RADIAL_FISHEYE", 5), 10: ("THIN_PRISM_FISHEYE", 12)}


def read_cameras_binary(path):
    """{camera_id: Camera} of a ``cameras.bin``."""
    cameras = {}
    with open(path, "rb") as fh:
        (n,) = _read(fh, "Q")
        for _ in range(n):
            camera_id, model_id, width, height = _read(fh, "iiQQ")
            if model_id not in CAMERA_MODELS:
                raise ValueError(f"{path}: unknown camera model id {model_id}")
            name, nparams = CAMERA_MODELS[model_id]
            cameras[camera_id] = Camera(camera_id, name, width, height, np.array(_read(fh, f"{nparams}d")))
    return cameras


def read_images_binary(path):
    """{image_id: Image} of an ``images.bin``."""
    images = {}
    with open(path, "rb") as fh:
        (n,) = _read(fh, "Q")
        for _ in range(n):
            image_id, qw, qx, qy, qz, tx, ty, tz, camera_id = _read(fh, "I7dI")
            name = bytearray()
            while True:
                c = fh.read(1)
                if c == b"":
                    raise ValueError(f"{path}: truncated image name")
                if c == b"\x00":
                    break
                name += c
            (npts,) = _read(fh, "Q")
            rec = np.frombuffer(fh.read(24 * npts), dtype=[("x", "<f8"), ("y", "<f8"), ("id", "<i8")], count=npts)
            images[image_id] = Image(image_id, np.array([qw, qx, qy, qz]), np.array([tx, ty, tz]), camera_id, name.decode("utf-8"),
                                     np.stack((rec["x"], rec["y"]), axis=1), rec["id"].copy())
    return images


def read_points3D_binary(path):
    """{point3D_id: Point3D} of a ``points3D.bin``."""
    points = {}
    with open(path, "rb") as fh:
        (n,) = _read(fh, "Q")
        for _ in range(n):
            pid, x, y, z, r, g, b, err, tlen = _read(fh, "Q3d3BdQ")
            track = np.frombuffer(fh.read(8 * tlen), dtype="<u4", count=2 * tlen).reshape(-1, 2)
            points[pid] = Point3D(pid, np.array([x, y, z]), np.array([r, g, b], dtype=np.uint8), err, track[:, 0].astype(np.int64),
                                  track[:, 1].astype(np.int64))
    return points


def shared_point_counts(model_dir, names):
    """[V,V] int64: the number of 3-D points of the sparse model at ``model_dir`` that images ``names[u]`` and ``names[v]`` both
    observe (diagonal 0).  Images of the model that are not in ``names`` are ignored."""
    model_dir = Path(model_dir)
    images = read_images_binary(model_dir / "images.bin")
    points = read_points3D_binary(model_dir / "points3D.bin")
    index = {name: k for k, name in enumerate(names)}
    by_id = {im.id: index[im.name] for im in images.values() if im.name in index}
    counts = np.zeros((len(names), len(names)), dtype=np.int64)
    for p in points.values():
        views = sorted({by_id[i] for i in p.image_ids.tolist() if i in by_id})
        for a in views:
            for b in views:
                if a != b:
                    counts[a, b] += 1
    return counts


def overlap_from_counts(counts, check_num_images: int = 50):
    """COLMAP's overlapping images per view: the views sharing at least one point, by shared count descending, ties by index,
    at most ``check_num_images`` of them."""
    out = []
    for v in range(counts.shape[0]):
        others = [u for u in range(counts.shape[0]) if u != v and counts[v, u] > 0]
        out.append(sorted(others, key=lambda u: (-int(counts[v, u]), u))[:check_num_images])
    return out


def overlap_from_covisibility(counts, check_num_images: int = 50, min_share: float = 0.0):
    """The overlap lists of ``overlap_from_counts`` from the [V,V,2] counts of ``ops.view_covisibility`` (a tensor or an array):
    view u is in v's list when ``counts[v,u,1]`` (the samples of v consistent with u's depth map) is positive and at least
    ``min_share`` x the number of valid samples of v; ordered by that count as ``overlap_from_counts`` orders shared points.  The
    number of valid samples of v is not an input: every valid sample is seen by at most every other view, so it is taken as the
    largest seen count of v's row, ``max_u counts[v,u,0]``, which equals it as soon as one view sees all of v's samples and is a
    lower bound (a more permissive share) otherwise.  A view with no valid depth gets an empty list."""
    c = np.asarray(counts.cpu() if hasattr(counts, "cpu") else counts).astype(np.int64)
    if c.ndim != 3 or c.shape[0] != c.shape[1] or c.shape[2] != 2:
        raise ValueError(f"overlap_from_covisibility: counts [V,V,2] expected, got {c.shape}")
    consistent = c[:, :, 1].copy()
    if min_share > 0.0:
        n_samples = c[:, :, 0].max(axis=1, keepdims=True)
        consistent[consistent < min_share * n_samples] = 0
    np.fill_diagonal(consistent, 0)
    return overlap_from_counts(consistent, check_num_images)
