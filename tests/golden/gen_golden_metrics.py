#!/usr/bin/env python3
"""Generate tests/golden/metrics_tiny.npz with the reference's own ``evaluation/metrics.py`` functions on small clouds:
``reduce_pts`` (seeded; the permutation it draws is recorded), ``chamfer_imw``, ``chamfer``, ``eval_dtu`` (``load_gt`` stubbed
with a small ObsMask, bounding box and plane) and ``eval_yfcc``.

The reference module needs two shims on a current stack: ``h5py`` is stubbed (gen_golden.import_reference), and scipy >= 1.9
spells cKDTree's ``n_jobs`` as ``workers``, so the module's ``cKDTree`` is replaced by a subclass that maps one to the other.
On numpy >= 2 an array has a ``.device`` attribute, so ``utils_3D.add_hom`` takes its torch branch and fails on a numpy array;
the module's ``add_hom`` is pointed at that function's own numpy branch (float64 ones appended), which older numpy took.
Runs ONLY where the reference tree is available.  Usage:  python tests/golden/gen_golden_metrics.py"""
from __future__ import annotations

import os
import pickle
import sys
import tempfile
from argparse import Namespace
from pathlib import Path

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from gen_golden import import_reference  # noqa: E402

SEED = 20261016


def clouds():
    """The fixed inputs (mm scale, like DTU): a clustered prediction with near-duplicates, outliers and points outside the box;
    a GT cloud with a region the prediction leaves empty."""
    rng = np.random.default_rng(SEED)
    surf = rng.uniform([0, 0, 0], [170, 150, 40], size=(900, 3))
    surf[:, 2] = 20 + 10 * np.sin(surf[:, 0] / 30.0)
    dup = surf[rng.integers(0, 900, 1500)] + rng.normal(0.0, 0.12, (1500, 3))
    far = rng.uniform([-80, -80, -60], [260, 240, 160], size=(200, 3))
    pred = np.concatenate((surf, dup, far)).astype(np.float32)
    gt = rng.uniform([0, 0, 0], [190, 150, 40], size=(2000, 3))
    gt[:, 2] = 20 + 10 * np.sin(gt[:, 0] / 30.0) + rng.normal(0.0, 0.3, 2000)
    gt = gt.astype(np.float32)
    bb = np.array([[-10.0, -12.5, -7.25], [190.0, 170.0, 150.0]])
    res = np.array([[4.0]])
    mask = rng.random((52, 47, 40)) < 0.7
    plane = np.array([[0.01], [0.02], [1.0], [-25.0]])
    small_from = rng.uniform(0, 10, size=(1500, 3)).astype(np.float32)
    small_to = rng.uniform(0, 10, size=(1200, 3)).astype(np.float32)
    return dict(pred=pred, gt=gt, bb=bb, res=res, obsmask=mask, plane=plane, small_from=small_from, small_to=small_to)


def main():
    import_reference()
    from scipy.spatial import cKDTree
    import evaluation.metrics as M

    class Tree(cKDTree):
        def query(self, *a, n_jobs=None, **k):
            return super().query(*a, **({"workers": n_jobs} if n_jobs else {}), **k)

        def query_ball_point(self, *a, n_jobs=None, **k):
            return super().query_ball_point(*a, **({"workers": n_jobs} if n_jobs else {}), **k)

    M.cKDTree = Tree
    M.add_hom = lambda pts: np.concatenate((pts, np.ones((pts.shape[0], 1))), axis=1)
    c = clouds()
    out = dict(c)

    np.random.seed(SEED)
    perm = np.random.permutation(c["pred"].shape[0])
    np.random.seed(SEED)
    _, mask = M.reduce_pts(c["pred"], 0.2)
    np.random.seed(SEED)
    _, mask_chunked = M.reduce_pts(c["pred"], 0.2, chunked=True)
    assert np.array_equal(mask, mask_chunked)
    out.update(reduce_perm=perm, reduce_mask=mask, reduce_dst=np.float64(0.2), seed=np.int64(SEED))

    out["imw_maxdist"] = np.float64(0.35)
    out["imw_dist"] = M.chamfer_imw(c["small_from"], c["small_to"], maxdist=0.35)
    out["chamfer_gt_to_pred"] = M.chamfer(c["gt"], c["pred"], c["bb"], 60)
    out["chamfer_pred_to_gt"] = M.chamfer(c["pred"], c["gt"], c["bb"], 60)

    M.load_gt = lambda scene, path: (c["gt"], c["obsmask"], c["bb"], c["res"], c["plane"])
    with tempfile.TemporaryDirectory() as td:
        args = Namespace(scene="scan1", data_path=td, chunked_eval=False)
        np.random.seed(SEED)
        M.eval_dtu(c["pred"], 0.2, Path(td) / "out", args)
        with open(Path(td) / "out" / "distsscan1.pkl", "rb") as fh:
            dtu = pickle.load(fh)
        # eval_yfcc reads data/yfcc_subset_dataset/gt_resolution/<scene>.txt relative to the working directory
        res_dir = Path(td) / "data" / "yfcc_subset_dataset" / "gt_resolution"
        res_dir.mkdir(parents=True)
        (res_dir / "sceneA.txt").write_text("0.05\n")
        (Path(td) / "Points" / "gt").mkdir(parents=True)
        from utils.utils_ply import write_ply
        write_ply(str(Path(td) / "Points" / "gt" / "sceneA_gt.ply"), [c["small_to"]], ["x", "y", "z"])
        cwd = os.getcwd()
        os.chdir(td)
        try:
            M.eval_yfcc(c["small_from"], Path(td) / "yout", Namespace(scene="sceneA_3", data_path=td))
        finally:
            os.chdir(cwd)
        with open(Path(td) / "yout" / "distssceneA_3.pkl", "rb") as fh:
            yfcc = pickle.load(fh)
    for k, v in dtu.items():
        out[f"dtu_{k}"] = np.asarray(v)
    for k, v in yfcc.items():
        out[f"yfcc_{k}"] = np.asarray(v)
    out["yfcc_res"] = np.float64(0.05)
    path = os.path.join(HERE, "metrics_tiny.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}  ({os.path.getsize(path) / 1024:.0f} KiB); kept {int(mask.sum())} of {mask.size}; "
          f"dtu pred kept {int(dtu['validMask'].size)}")


if __name__ == "__main__":
    main()
