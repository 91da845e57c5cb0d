#!/usr/bin/env python3
"""Generate the fixture of the scene set-up: a sparse model of 12 images and 300 points written with
the reference's own COLMAP writer to tests/golden/scene_tiny/{cameras,images,points3D}.bin, and what the reference's
``utils/colmap_utils.py`` makes of it -- ``get_calib_from_sparse``, ``compute_src_imgs(..., 5 degrees, nsrc=4, None)`` and
``compute_min_max_depth_yao`` -- in tests/golden/scene_tiny.npz (arrays only).

The model: two PINHOLE cameras, images on a jittered 4 x 3 rig 0.45 apart looking at points 3..7 away, so that neighbouring
pairs fail the 5-degree test and distant ones pass; tracks of 2..9 images; point 1000 names one image twice; image id 40 has
keypoints but no matched one; COLMAP ids follow neither the names nor the order.

The reference's answer must not rest on chance, so a seed is accepted only if
  * in every row of an image with observations the nsrc + 1 largest surviving counts are distinct and positive (no choice rests on
    a tie; the row of the image without observations is all zeros, where a stable sort -- numpy's for 12 elements is an
    insertion sort -- returns the last indices in order),
  * no pair's angle lies within 1e-3 degrees of the threshold (the reference multiplies in float32, the engine in float64),
  * every image but the empty one has at least 20 observations;
otherwise the next seed is tried.

Runs ONLY where the reference tree is available (imported the way gen_golden.py does).  The reference's function uses ``np.int``
and ``np.bool``, which current numpy no longer has: this script puts them back before the call.
Usage:  python tests/golden/gen_golden_scene.py"""
from __future__ import annotations

import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)
from gen_golden import import_reference  # noqa: E402

N_IMAGES, N_POINTS, NSRC, MIN_ANGLE = 12, 300, 4, 5.0
SPACING = 0.45                                # of the rig: neighbours fail the 5-degree test, diagonal neighbours pass
EMPTY = 7                                     # position of the image without a matched keypoint
IMAGE_IDS = [12, 3, 31, 8, 5, 19, 2, 40, 27, 14, 9, 22]


def make_model(rw, seed):
    from tests import _scene_setup_ref as SR
    rng = np.random.default_rng(seed)
    R, t = SR.rig(N_IMAGES, rng, SPACING)
    cameras = {1: rw.Camera(id=1, model="PINHOLE", width=640, height=480, params=np.array([520.0, 522.5, 320.0, 240.0])),
               4: rw.Camera(id=4, model="PINHOLE", width=512, height=384, params=np.array([410.0, 411.0, 255.5, 190.25]))}
    seen = np.array([k for k in range(N_IMAGES) if k != EMPTY])
    weight = rng.permutation(1.25 ** np.arange(len(seen)))           # spread the counts: fewer ties
    obs = {k: [] for k in range(N_IMAGES)}
    points = {}
    for n in range(N_POINTS):
        pid = 1000 + 3 * n
        track = rng.choice(seen, int(rng.integers(2, 10)), replace=False, p=weight / weight.sum()).tolist()
        if n == 0:
            track = track[:3] + track[:1]                        # this point's track names its first image twice
        idxs = []
        for k in track:
            idxs.append(len(obs[k]))
            obs[k].append(pid)
        xyz = np.array([rng.uniform(-2, 2), rng.uniform(-2, 2), rng.uniform(3, 7)])
        points[pid] = rw.Point3D(id=pid, xyz=xyz, rgb=rng.integers(0, 256, 3).astype(np.uint8), error=float(rng.random()),
                                 image_ids=np.array([IMAGE_IDS[k] for k in track]), point2D_idxs=np.array(idxs))
    quat = np.concatenate([np.ones((N_IMAGES, 1)), rng.normal(0, 0.03, (N_IMAGES, 3))], axis=1)
    quat /= np.linalg.norm(quat, axis=1, keepdims=True)
    centre = -np.einsum("nji,nj->ni", R.astype(np.float64), t.astype(np.float64))
    images = {}
    for k in range(N_IMAGES):
        ids = np.array(obs[k] + [-1, -1], dtype=np.int64)          # two unmatched keypoints each: the empty image has only those
        Rk = rw.qvec2rotmat(quat[k])
        images[IMAGE_IDS[k]] = rw.Image(id=IMAGE_IDS[k], qvec=quat[k], tvec=-Rk @ centre[k], camera_id=1 if k % 3 else 4,
                                        name=f"{k:08d}.jpg", xys=rng.random((len(ids), 2)) * 300, point3D_ids=ids)
    return cameras, images, points


def main():
    import_reference()
    if "tqdm" not in sys.modules:
        try:
            import tqdm  # noqa: F401
        except Exception:
            sys.modules["tqdm"] = types.ModuleType("tqdm")
            sys.modules["tqdm"].tqdm = lambda it, **kw: it
    import utils.read_write_model_colmap as rw
    import utils.colmap_utils as ref
    from tests import _scene_setup_ref as SR
    np.int, np.bool = int, bool                                    # (removed from numpy 1.24; the reference still spells them)
    out = os.path.join(HERE, "scene_tiny")
    os.makedirs(out, exist_ok=True)
    for seed in range(20261018, 20261018 + 4000):
        cameras, images, points = make_model(rw, seed)
        K, R, t, sizes = ref.get_calib_from_sparse(cameras, images)
        mine = SR.scene_setup(images, points, R, t, min_triangulation_angle=MIN_ANGLE, nsrc=NSRC)
        common = np.where(4 * mine["adj_tri"] < 3 * mine["adj"], 0, mine["adj"])
        top = np.sort(common, axis=1)[:, -(NSRC + 1):]
        rows = np.arange(N_IMAGES) != EMPTY
        no_tie = bool((top[rows, 0] > 0).all() and (np.diff(top[rows], axis=1) > 0).all())
        n_obs = np.array([(im.point3D_ids != -1).sum() for im in images.values()])
        enough = bool((n_obs[rows] >= 20).all()) and n_obs[EMPTY] == 0
        if no_tie and mine["margin"] > 1e-3 and enough and not common[EMPTY].any():
            print(f"seed {seed}: no tie, angle margin {mine['margin']:.3e} deg, observations {n_obs.tolist()}")
            break
    else:
        raise SystemExit("no seed met the three conditions")
    rw.write_model(cameras, images, points, out, ext=".bin")
    cameras, images, points = rw.read_model(out, ext=".bin")                   # what the tests will read: doubles survive the file
    K, R, t, sizes = ref.get_calib_from_sparse(cameras, images)
    again = SR.scene_setup(images, points, R, t, min_triangulation_angle=MIN_ANGLE, nsrc=NSRC)
    assert all(np.array_equal(again[k], mine[k]) for k in ("adj", "adj_tri", "depth_min", "depth_max")) and again["margin"] == mine["margin"]
    sel = ref.compute_src_imgs(images, points, R, t, MIN_ANGLE, NSRC, None)
    dmin, dmax, _, _ = ref.compute_min_max_depth_yao(points, images, K, R, t)
    tri = mine["adj_tri"][~np.eye(N_IMAGES, dtype=bool) & (mine["adj"] > 0)]
    share = mine["adj_tri"] / np.maximum(mine["adj"], 1)
    assert (share[mine["adj"] > 0] < 0.75).sum() > N_IMAGES and (share >= 0.75).sum() > N_IMAGES, "the rig: some pairs pass, some fail"
    assert sel == mine["sel_idx"], "the restatement disagrees with the reference"
    assert np.allclose(dmin, mine["depth_min"], rtol=1e-12, atol=0) and np.allclose(dmax, mine["depth_max"], rtol=1e-12, atol=0)
    assert dmin[EMPTY] == 0 and dmax[EMPTY] == 0
    path = os.path.join(HERE, "scene_tiny.npz")
    np.savez_compressed(path, sel_idx=np.array(sel, dtype=np.int64), depth_min=dmin, depth_max=dmax, K=K, R=R, t=t, sizes=sizes,
                        min_triangulation_angle=np.float64(MIN_ANGLE), nsrc=np.int64(NSRC), empty_image=np.int64(EMPTY),
                        seed=np.int64(seed))
    print(f"wrote {out} and {path}: pairs with a shared point {len(tri)}, of which {int((tri > 0).sum())} have a point past "
          f"{MIN_ANGLE} degrees; sel_idx[0] = {sel[0]}")


if __name__ == "__main__":
    main()
