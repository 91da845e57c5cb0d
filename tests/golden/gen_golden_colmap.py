#!/usr/bin/env python3
"""Generate tests/golden/colmap_tiny/{cameras,images,points3D}.bin with the reference's own COLMAP model writer
(``utils/read_write_model_colmap.py:write_model``) for a fixed tiny model: 4 images, 6 points with tracks of 2-4 images.
tests/test_colmap_fusion_cpu.py reads it back with wild_deep_mvs_amd/utils/colmap_model.py.

Runs ONLY where the reference tree is available (imported the way gen_golden.py does).
Usage:  python tests/golden/gen_golden_colmap.py"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from gen_golden import import_reference  # noqa: E402

NAMES = ["00000000.jpg", "00000001.jpg", "00000002.jpg", "00000003.jpg"]
IMAGE_IDS = [3, 1, 7, 2]                     # COLMAP ids need not follow the names
TRACKS = [[3, 1], [3, 1, 7], [1, 7], [3, 1, 7, 2], [7, 2], [3, 7]]   # image ids observing each point


def main():
    import_reference()
    import utils.read_write_model_colmap as rw
    rng = np.random.default_rng(20261016)
    cameras = {1: rw.Camera(id=1, model="PINHOLE", width=32, height=24, params=np.array([28.8, 28.8, 16.0, 12.0]))}
    obs = {i: [] for i in IMAGE_IDS}
    points = {}
    for pid, track in enumerate(TRACKS, start=10):
        idxs = []
        for i in track:
            idxs.append(len(obs[i]))
            obs[i].append(pid)
        points[pid] = rw.Point3D(id=pid, xyz=rng.standard_normal(3), rgb=rng.integers(0, 256, 3).astype(np.uint8),
                                 error=float(rng.random()), image_ids=np.array(track), point2D_idxs=np.array(idxs))
    images = {}
    for name, i in zip(NAMES, IMAGE_IDS):
        pts = np.array(obs[i] + [-1], dtype=np.int64)          # one unmatched keypoint each
        images[i] = rw.Image(id=i, qvec=np.array([1.0, 0.0, 0.0, 0.0]), tvec=rng.standard_normal(3), camera_id=1, name=name,
                             xys=rng.random((len(pts), 2)) * 20, point3D_ids=pts)
    out = os.path.join(HERE, "colmap_tiny")
    os.makedirs(out, exist_ok=True)
    rw.write_model(cameras, images, points, out, ext=".bin")
    print(f"wrote {out}")


if __name__ == "__main__":
    main()
