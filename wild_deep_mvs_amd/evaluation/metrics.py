"""Point-cloud metrics on MI355X -- drop-in for ``evaluation/metrics.py`` of fdarmon/wild_deep_mvs.

The reference runs scipy ``cKDTree`` queries on the host (and, on a current SciPy, fails on their ``n_jobs`` keyword).  Here the
three searches are HIP kernels (``csrc/point_metrics.hip``; INTEGRATION.md section 2f states the rules):

- ``reduce_pts`` is the greedy maximal independent set of the radius graph in the order of ``np.random.permutation(n)``, run
  as parallel rounds (``ops.radius_downsample``); for a given ``np.random.seed`` it keeps the points upstream keeps;
- ``chamfer_imw`` / ``chamfer`` are bounded nearest-neighbour distances (``ops.nn_dist``), the latter with the reference's
  blocking by cells of ``maxdist``.

``run(args)`` keeps the reference's interface, paths and pickle contents.  Neither SciPy nor ``h5py`` is imported here: only
``load_gt`` needs ``scipy.io.loadmat`` (DTU's ObsMask files) and imports it when called.
"""
from __future__ import annotations

import pickle
import time
from pathlib import Path

import numpy as np
import torch

from .. import ops
from ..utils.point_cloud import read_ply
from .filtering import depth_folder_name

DEVICE = "cuda"


def format_point_cloud(ply):
    pts = np.stack((ply["x"], ply["y"], ply["z"]), axis=1)
    return pts[~(np.isnan(pts).any(axis=1))]


def _gpu_points(pts, what):
    pts = np.asarray(pts)
    if pts.dtype != np.float32 or pts.ndim != 2 or pts.shape[1] != 3:
        raise ValueError(f"metrics.{what}: float32 [n,3] points expected (as read_ply gives them), got {pts.dtype} {pts.shape}")
    return torch.from_numpy(np.ascontiguousarray(pts)).to(DEVICE)


def reduce_pts(pts, dst, chunked=False):
    """Keep a maximal set of points no two of which lie within ``dst`` (inclusive): upstream's greedy pass in the order of
    ``np.random.permutation(n)``, drawn here exactly as upstream draws it, so the same seed keeps the same points.  ``chunked``
    is accepted and ignored: upstream's two branches give the same mask, and the GPU rounds need no chunking.
    Returns ``(pts[mask], mask)``."""
    n = pts.shape[0]
    rand_ord = np.random.permutation(n)
    rank = np.empty(n, dtype=np.int32)
    rank[rand_ord] = np.arange(n, dtype=np.int32)
    with torch.no_grad():
        _, mask, _ = ops.radius_downsample(_gpu_points(pts, "reduce_pts"), dst, torch.from_numpy(rank).to(DEVICE))
    mask = mask.cpu().numpy()
    return pts[mask], mask


def load_gt(scene_name, path):
    from scipy.io import loadmat          # (only here: the GPU hosts need not have SciPy)
    scene = int(scene_name[4:])
    loaded = loadmat(path / "ObsMask" / f"ObsMask{scene}_10.mat")
    bb, mask, res = loaded["BB"], loaded["ObsMask"], loaded["Res"]
    plane = loadmat(path / "ObsMask" / f"Plane{scene}.mat")["P"]
    point_cloud = format_point_cloud(read_ply(path / "Points" / "stl" / f"stl{scene:03d}_total.ply"))
    return point_cloud, mask, bb, res, plane


def eval_yfcc(pred_pts, out_path, args):
    scene = "_".join(args.scene.split("_")[:-1])
    res = np.loadtxt(Path("data/yfcc_subset_dataset/gt_resolution") / f"{scene}.txt").squeeze()
    gt_pts = format_point_cloud(read_ply(Path(args.data_path) / "Points" / "gt" / f"{scene}_gt.ply"))
    dist_gtToPred = chamfer_imw(gt_pts, pred_pts, maxdist=10 * res)
    dist_predToGt = chamfer_imw(pred_pts, gt_pts, maxdist=10 * res)
    res = {
        "dist_gtToPred": dist_gtToPred,
        "dist_predToGt": dist_predToGt
    }
    if not out_path.exists():
        out_path.mkdir(parents=True)
    with open(out_path / f"dists{args.scene}.pkl", "wb") as f:
        pickle.dump(res, f)


def chamfer_imw(pts_from, pts_to, maxdist=np.inf):
    """float64 [n_from]: distance to the nearest ``pts_to`` point when strictly below ``maxdist``, else inf."""
    with torch.no_grad():
        d = ops.nn_dist(_gpu_points(pts_from, "chamfer_imw"), _gpu_points(pts_to, "chamfer_imw"), float(maxdist))
    return d.cpu().numpy()


def eval_dtu(pred_pts, dst, outPath, args):
    # reimplementation of DTU evaluation matlab code (as upstream; it does not guarantee the matlab code's exact results)
    margin = 10
    maxdist = 60
    print(f"Removing duplicated points within a radius of {dst}")
    start = time.time()
    pred_pts, _ = reduce_pts(pred_pts, dst, chunked=getattr(args, "chunked_eval", False))
    print(f"Done in {time.time() - start}s")

    gt_pts, mask, bb, res, plane = load_gt(args.scene, Path(args.data_path))

    abovePlane = (np.concatenate((gt_pts, np.ones((gt_pts.shape[0], 1))), axis=1) @ plane) > 0
    normalized_pts = np.rint((pred_pts - bb[0:1]) / res).astype(int)

    valid1 = (normalized_pts >= 0).all(axis=1) & (normalized_pts < np.array(mask.shape)[None]).all(axis=1)
    normalized_pts = normalized_pts[valid1]

    validMask = np.zeros((pred_pts.shape[0],), dtype=bool)
    valid2 = mask.astype(bool)[normalized_pts[:, 0], normalized_pts[:, 1], normalized_pts[:, 2]]
    validMask[np.where(valid1)[0][valid2]] = True

    print("Computing distance from GT to Pred")
    dist_gtToPred = chamfer(gt_pts, pred_pts, bb, maxdist)
    print("Computing distance from Pred to GT")
    dist_predToGt = chamfer(pred_pts, gt_pts, bb, maxdist)

    res = {
        "margin": margin,
        "maxdist": maxdist,
        "abovePlane": abovePlane,
        "validMask": validMask,
        "dist_gtToPred": dist_gtToPred,
        "dist_predToGt": dist_predToGt
    }
    if not outPath.exists():
        outPath.mkdir(parents=True)
    with open(outPath / f"dists{args.scene}.pkl", "wb") as f:
        pickle.dump(res, f)


def chamfer(ptsFrom, ptsTo, bb, maxdist):
    """Upstream's blocked distance: float64 [n_from], ``maxdist`` for a point in no cell of ``bb`` or whose cell's expanded box
    holds no ``ptsTo`` point, otherwise the distance to the nearest ``ptsTo`` point of that box when below ``maxdist``, else inf."""
    with torch.no_grad():
        d = ops.nn_dist(_gpu_points(ptsFrom, "chamfer"), _gpu_points(ptsTo, "chamfer"), float(maxdist),
                        bb=np.asarray(bb, dtype=np.float64))
    return d.cpu().numpy()


def run(args):
    folder_name = depth_folder_name(args)
    points_path = Path(args.data_path) / "Points" / folder_name
    pred_pts = format_point_cloud(read_ply(points_path / f"{folder_name}{args.scene}.ply"))

    outPath = Path(args.data_path) / "IntRes" / "chamfer" / folder_name
    if (outPath / f"dists{args.scene}.pkl").exists() and not getattr(args, "override_fusion", False):
        print("Chamfer already computed, continue...")
        return

    if args.dataset == "dtu":
        eval_dtu(pred_pts, 0.2, outPath, args)
    else:
        eval_yfcc(pred_pts, outPath, args)


# ---------------------------------------------------------------------------------------------------------------------------
# Scoring a triangle mesh: an addition of this project, the reference has no counterpart.  The mesh is
# sampled proportionally to its area (``ops.mesh_sample``) and the samples take the place of the fused cloud; the completeness
# direction can use the exact distance to the surface (``ops.mesh_dist``) instead of the distance to the nearest sample.
def _gpu_mesh(xyz, faces, what):
    xyz, faces = np.asarray(xyz), np.asarray(faces)
    if xyz.dtype != np.float32 or xyz.ndim != 2 or xyz.shape[1] != 3:
        raise ValueError(f"metrics.{what}: float32 [V,3] vertices expected (as read_mesh gives them), got {xyz.dtype} {xyz.shape}")
    if faces.dtype != np.int32 or faces.ndim != 2 or faces.shape[1] != 3:
        raise ValueError(f"metrics.{what}: int32 [F,3] faces expected (as read_mesh gives them), got {faces.dtype} {faces.shape}")
    return torch.from_numpy(np.ascontiguousarray(xyz)).to(DEVICE), torch.from_numpy(np.ascontiguousarray(faces)).to(DEVICE)


def sample_mesh(xyz, faces, spacing, seed=0):
    """(samples float32 [N,3], face int32 [N]): deterministic samples of the mesh's surface, on average one per ``spacing``^2 of
    area, and the face each lies on (``ops.mesh_sample``; numpy in, numpy out)."""
    with torch.no_grad():
        pts, face = ops.mesh_sample(*_gpu_mesh(xyz, faces, "sample_mesh"), float(spacing), seed=int(seed), return_faces=True)
    return pts.cpu().numpy(), face.cpu().numpy()


def mesh_to_cloud_dists(xyz, faces, gt_pts, maxdist, *, spacing, completeness="surface", bb=None, reduce_dst=None, seed=0):
    """Both Chamfer directions between a triangle mesh and a ground-truth cloud -> dict(samples, dist_predToGt, dist_gtToPred).

    The mesh is sampled (``sample_mesh``) and, with ``reduce_dst``, thinned by ``reduce_pts``; ``dist_predToGt`` is ``chamfer``
    (with ``bb``, DTU) or ``chamfer_imw`` (without) from the samples to ``gt_pts``.  ``dist_gtToPred`` is, with ``completeness``
    = "samples", the same function from ``gt_pts`` to the samples -- exactly what today's evaluation gives on that cloud -- and
    with "surface" (the default) ``ops.mesh_dist``: the exact distance to the surface when strictly below ``maxdist``, else inf.
    Under DTU this differs from ``chamfer``'s block rule, which gives ``maxdist`` itself to a point in no cell or in a cell whose
    expanded box is empty: in "surface" mode such a point gets inf.  Both values mean "not below maxdist"."""
    if completeness not in ("surface", "samples"):
        raise ValueError(f"metrics.mesh_to_cloud_dists: completeness must be 'surface' or 'samples', got {completeness!r}")
    samples, _ = sample_mesh(xyz, faces, spacing, seed)
    if reduce_dst is not None:
        samples, _ = reduce_pts(samples, reduce_dst)
    dist = (lambda a, b: chamfer_imw(a, b, maxdist=maxdist)) if bb is None else (lambda a, b: chamfer(a, b, bb, maxdist))
    dist_predToGt = dist(samples, gt_pts)
    if completeness == "samples":
        dist_gtToPred = dist(gt_pts, samples)
    else:
        gxyz, gfaces = _gpu_mesh(xyz, faces, "mesh_to_cloud_dists")
        with torch.no_grad():
            dist_gtToPred = ops.mesh_dist(_gpu_points(gt_pts, "mesh_to_cloud_dists"), gxyz, gfaces, float(maxdist)).cpu().numpy()
    return {"samples": samples, "dist_predToGt": dist_predToGt, "dist_gtToPred": dist_gtToPred}


def _mesh_options(args, default_spacing):
    spacing = getattr(args, "mesh_sample_spacing", None)
    return dict(spacing=float(default_spacing if spacing is None else spacing),
                completeness=getattr(args, "mesh_completeness", None) or "surface", seed=int(getattr(args, "mesh_sample_seed", 0) or 0))


def eval_dtu_mesh(xyz, faces, dst, outPath, args):
    """``eval_dtu`` for a mesh: the same pickle keys, ``validMask`` and ``abovePlane`` computed on the (thinned) samples exactly as
    ``eval_dtu`` computes them on the cloud.  The default sample spacing is half the downsampling radius ``dst``."""
    margin = 10
    maxdist = 60
    gt_pts, mask, bb, res, plane = load_gt(args.scene, Path(args.data_path))
    d = mesh_to_cloud_dists(xyz, faces, gt_pts, maxdist, bb=bb, reduce_dst=dst, **_mesh_options(args, 0.5 * dst))
    pred_pts = d["samples"]

    abovePlane = (np.concatenate((gt_pts, np.ones((gt_pts.shape[0], 1))), axis=1) @ plane) > 0
    normalized_pts = np.rint((pred_pts - bb[0:1]) / res).astype(int)

    valid1 = (normalized_pts >= 0).all(axis=1) & (normalized_pts < np.array(mask.shape)[None]).all(axis=1)
    normalized_pts = normalized_pts[valid1]

    validMask = np.zeros((pred_pts.shape[0],), dtype=bool)
    valid2 = mask.astype(bool)[normalized_pts[:, 0], normalized_pts[:, 1], normalized_pts[:, 2]]
    validMask[np.where(valid1)[0][valid2]] = True

    res = {
        "margin": margin,
        "maxdist": maxdist,
        "abovePlane": abovePlane,
        "validMask": validMask,
        "dist_gtToPred": d["dist_gtToPred"],
        "dist_predToGt": d["dist_predToGt"]
    }
    if not outPath.exists():
        outPath.mkdir(parents=True)
    with open(outPath / f"dists{args.scene}.pkl", "wb") as f:
        pickle.dump(res, f)


def eval_yfcc_mesh(xyz, faces, out_path, args):
    """``eval_yfcc`` for a mesh: the same pickle keys; the default sample spacing is the scene's resolution."""
    scene = "_".join(args.scene.split("_")[:-1])
    res = float(np.loadtxt(Path("data/yfcc_subset_dataset/gt_resolution") / f"{scene}.txt").squeeze())
    gt_pts = format_point_cloud(read_ply(Path(args.data_path) / "Points" / "gt" / f"{scene}_gt.ply"))
    d = mesh_to_cloud_dists(xyz, faces, gt_pts, 10 * res, **_mesh_options(args, res))
    res = {
        "dist_gtToPred": d["dist_gtToPred"],
        "dist_predToGt": d["dist_predToGt"]
    }
    if not out_path.exists():
        out_path.mkdir(parents=True)
    with open(out_path / f"dists{args.scene}.pkl", "wb") as f:
        pickle.dump(res, f)


def run_mesh(args):
    """``run`` for the mesh that ``tsdf_fusion.run`` writes: reads ``<data_path>/Meshes/<folder>/<folder><scene>.ply`` and writes
    ``<data_path>/IntRes/chamfer_mesh/<folder>/dists<scene>.pkl``.  Opt-in: nothing else calls it.  ``args.mesh_sample_spacing``
    (default: 0.1 for DTU, the scene's resolution for YFCC), ``args.mesh_completeness`` ("surface" / "samples") and
    ``args.mesh_sample_seed`` are optional."""
    from ..utils.point_cloud import read_mesh
    folder_name = depth_folder_name(args)
    xyz, _, faces = read_mesh(Path(args.data_path) / "Meshes" / folder_name / f"{folder_name}{args.scene}.ply")

    outPath = Path(args.data_path) / "IntRes" / "chamfer_mesh" / folder_name
    if (outPath / f"dists{args.scene}.pkl").exists() and not getattr(args, "override_fusion", False):
        print("Chamfer already computed, continue...")
        return

    if args.dataset == "dtu":
        eval_dtu_mesh(xyz, faces, 0.2, outPath, args)
    else:
        eval_yfcc_mesh(xyz, faces, outPath, args)
