"""COLMAP-style stereo fusion on MI355X -- drop-in for ``utils/colmap_utils.py:colmap_fusion`` of fdarmon/wild_deep_mvs.

The reference writes COLMAP workspace files and runs the external ``colmap image_undistorter`` and ``colmap stereo_fusion``
binaries (``utils/colmap_utils.py:324-400``), which are not part of the AMD stack.  Here the fusion is ``pscv_colmap_fuse_pass``,
two HIP phases per view (INTEGRATION.md section 2g states the rule and its named deviations from COLMAP; it restates
StereoFusion as the reference configures it -- ``max_depth_error``, ``max_reproj_error`` and ``min_num_pixels`` from the command
line, COLMAP's defaults for the rest -- and has not been compared with the binary).

``colmap_fusion(dataloader, args)`` keeps the reference's interface and writes the file its metrics step reads,
``<data_path>/Points/<model>_<nviews>/<model>_<nviews><scene>.ply``, in COLMAP's fused PLY layout.

Network path (``args.colmap`` false): constant normals, the normal test off (``max_normal_error 180`` in the reference).  With
``args.fusion_normals = "depth"`` the normal maps come from the masked depth maps themselves (``ops.depth_normals``, INTEGRATION.md
section 2n) and the normal test runs at ``args.fusion_max_normal_error`` (default 180 degrees: every pair passes, the points are
the default run's and carry real normals).
COLMAP baseline (``args.colmap``): the geometric normal maps that ``depthmap_colmap`` wrote under
``IntRes/colmap_dense/<scene>/stereo/normal_maps`` go into ``pscv_colmap_fuse_pass_normals`` with ``MAX_NORMAL_ERROR`` = 10
degrees; until that folder exists the call raises ``NotImplementedError`` and touches no file.
"""
from __future__ import annotations

from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

from .. import ops
from ..utils.colmap_array import read_array
from ..utils.colmap_model import overlap_from_counts, overlap_from_covisibility, shared_point_counts
from ..utils.point_cloud import write_colmap_point_cloud
from .filtering import depth_folder_name
from .fusibile import depth_normal_options, get_mask, normal_source

CHECK_NUM_IMAGES = 50          # COLMAP's StereoFusionOptions defaults
MAX_TRAVERSAL_DEPTH = 100
MAX_NUM_PIXELS = 10000
MAX_NORMAL_ERROR = 10.0        # degrees, under args.colmap: "--StereoFusion.max_normal_error 10" (utils/colmap_utils.py:396)


def nearest_colors(img: torch.Tensor, h: int, w: int) -> np.ndarray:
    """[3,H,W] image in [0,1] -> uint8 [h,w,3]: x 255 truncated to a byte (ToPILImage), sampled nearest-neighbour at the image
    position (col W / w, row H / h) of each depth-map pixel, rounded half away from zero and clamped (COLMAP's
    InterpolateNearestNeighbor with its bitmap scale)."""
    H, W = img.shape[1:]
    arr = img.detach().cpu().mul(255).byte().permute(1, 2, 0).numpy()
    xs = np.minimum(np.floor(np.arange(w) * (W / w) + 0.5).astype(np.int64), W - 1)
    ys = np.minimum(np.floor(np.arange(h) * (H / h) + 0.5).astype(np.int64), H - 1)
    return np.ascontiguousarray(arr[ys[:, None], xs[None, :]])


def view_inputs(args, batch, depth_file):
    """(masked depth, colours, K at the depth map's size, R, t) of a batch's view 0, as colmap_fusion prepares its workspace."""
    filename = batch["filename"][0]
    npz = np.load(depth_file)
    depth, prob = np.array(npz["depthmap"], dtype=np.float32), np.array(npz["probability"], dtype=np.float32)
    if args.upsample:
        up = lambda a: F.interpolate(torch.from_numpy(a)[None, None], mode="bilinear", scale_factor=args.downscale,
                                     align_corners=False)[0, 0].numpy()
        depth, prob = up(depth), up(prob)
    depth[get_mask(args, filename, prob)] = 0
    img = batch["imgs"][0, 0]
    h_img, w_img = img.shape[1:]
    h_d, w_d = depth.shape
    K = batch["K"][0, 0].clone().to(torch.float64)
    K[0] *= w_d / w_img
    K[1] *= h_d / h_img
    return (np.ascontiguousarray(depth), nearest_colors(img, h_d, w_d), K.to(torch.float32), batch["R"][0, 0].to(torch.float32),
            batch["t"][0, 0].to(torch.float32).reshape(3, 1))


OVERLAP_SOURCES = ("auto", "sparse", "all", "depth")


def scene_overlap(args, names, depths=None, cams=None):
    """COLMAP's overlapping images of every view, from the source ``args.fusion_overlap`` names (default "auto"):
      "auto"    the sparse model at IntRes/colmap_sparse/<scene> when there is one (shared 3-D points, descending, ties by index,
                at most CHECK_NUM_IMAGES), else every other view;
      "sparse"  the sparse model, which has to be there;
      "all"     every other view (the first CHECK_NUM_IMAGES by index);
      "depth"   the views whose depth maps agree ("Overlap without a sparse model"):
                ``ops.view_covisibility`` over ``depths`` (the masked maps on the GPU, the ones the fusion reads) and ``cams`` with
                ``args.fusion_depth_threshold`` and ``args.fusion_overlap_stride`` (default 4), consistent samples descending.
    -> (lists, description of the source)."""
    mode = getattr(args, "fusion_overlap", "auto")
    if mode not in OVERLAP_SOURCES:
        raise ValueError(f"colmap_fusion: fusion_overlap must be one of {OVERLAP_SOURCES}, got {mode!r}")
    n = len(names)
    if mode == "depth":
        if depths is None or cams is None:
            raise ValueError("colmap_fusion: fusion_overlap 'depth' needs the depth maps and cameras on the GPU")
        stride = int(getattr(args, "fusion_overlap_stride", 4))
        counts = ops.view_covisibility(depths, cams, stride=stride, max_depth_error=args.fusion_depth_threshold)
        return overlap_from_covisibility(counts, CHECK_NUM_IMAGES), f"depth-map covisibility (stride {stride})"
    sparse = Path(args.data_path) / "IntRes" / "colmap_sparse" / str(args.scene)
    have = (sparse / "images.bin").exists() and (sparse / "points3D.bin").exists()
    if mode == "sparse" and not have:
        raise FileNotFoundError(f"colmap_fusion: fusion_overlap 'sparse' needs the sparse model {sparse} (images.bin, points3D.bin)")
    if have and mode != "all":
        counts = shared_point_counts(sparse, [name + ".jpg" for name in names])
        return overlap_from_counts(counts, CHECK_NUM_IMAGES), f"sparse model {sparse}"
    return ([[u for u in range(n) if u != v][:CHECK_NUM_IMAGES] for v in range(n)],
            "all other views" + (" (no sparse model)" if mode == "auto" else ""))


def view_normals(normal_dir, filename, shape):
    """The geometric normal map of one view (camera frame, fp32 [h,w,3]) at the depth map's size ``shape``; not resampled."""
    path = Path(normal_dir) / f"{filename}.jpg.geometric.bin"
    if not path.exists():
        raise FileNotFoundError(f"colmap_fusion: view {filename} has a depth map but no normal map {path}")
    normal = read_array(path)
    if normal.ndim != 3 or normal.shape[2] != 3 or normal.shape[:2] != tuple(shape):
        raise ValueError(f"colmap_fusion: normal map {path} is {normal.shape}, the depth map of view {filename} is {tuple(shape)} "
                         "(after args.upsample); normal maps are not resampled")
    return np.ascontiguousarray(normal, dtype=np.float32)


def colmap_fusion(dataloader, args):
    depth_normals = normal_source(args) == "depth"
    use_normals = bool(getattr(args, "colmap", False))
    normal_dir = Path(args.data_path) / "IntRes" / "colmap_dense" / str(args.scene) / "stereo" / "normal_maps"
    if use_normals and not normal_dir.is_dir():
        raise NotImplementedError(f"colmap_fusion with args.colmap fuses the depth and normal maps of depthmap_colmap, which has "
                                  f"to run first: {normal_dir} does not exist")
    folder_name = depth_folder_name(args)
    ply_dir = Path(args.data_path) / "Points" / folder_name
    outfile = ply_dir / f"{folder_name}{args.scene}.ply"
    if outfile.exists() and not args.override:
        print("Point cloud Fusion already done")
        return
    depth_folder = Path(args.data_path) / "IntRes" / "depthmaps" / folder_name / str(args.scene)
    if use_normals:
        # the reference reads IntRes/depthmaps/None_<nviews>/<scene> here, a folder none of its steps writes; depthmap_colmap
        # writes IntRes/direct_depthmaps/colmap/<scene> (INTEGRATION.md section 2g names the deviation)
        if not depth_folder.is_dir():
            depth_folder = Path(args.data_path) / "IntRes" / "direct_depthmaps" / "colmap" / str(args.scene)
        print(f"COLMAP fusion reads the depth maps of {depth_folder}")
    views, names, normals = [], [], []
    for b in dataloader:
        filename = b["filename"][0]
        depth_file = depth_folder / f"{filename}_out.npz"
        if not depth_file.exists():
            print(f"Could not open {depth_file}")          # the view is left out of the fusion, as in the reference
            continue
        views.append(view_inputs(args, b, depth_file))
        names.append(filename)
        if use_normals:
            normals.append(view_normals(normal_dir, filename, views[-1][0].shape))
    depths, colors, K, R, t = zip(*views)
    extra = dict(normals=[torch.from_numpy(n).cuda() for n in normals], max_normal_error=MAX_NORMAL_ERROR) if use_normals else {}
    with torch.no_grad():
        cams = ops.geo_filter_cams(torch.stack(K), torch.stack(R), torch.stack(t)).cuda()
        depths = [torch.from_numpy(d).cuda() for d in depths]          # uploaded once: the overlap pass and the fusion share them
        overlap, source = scene_overlap(args, names, depths, cams)
        print(f"COLMAP fusion of {len(views)} views, overlap from {source}")
        if depth_normals:                                              # from the maps the fusion reads, after upsample and mask
            extra = dict(normals=ops.depth_normals(depths, cams, **depth_normal_options(args)),
                         max_normal_error=getattr(args, "fusion_max_normal_error", 180.0))
        xyz, normal, rgb, _ = ops.colmap_fuse(depths, [torch.from_numpy(c).cuda() for c in colors],
                                              cams, overlap, max_depth_error=args.fusion_depth_threshold,
                                              max_reproj_error=args.fusion_max_reproj_error, min_num_pixels=args.fusion_num_consistent,
                                              max_traversal_depth=MAX_TRAVERSAL_DEPTH, max_num_pixels=MAX_NUM_PIXELS, **extra)
    ply_dir.mkdir(parents=True, exist_ok=True)
    write_colmap_point_cloud(outfile, xyz, normal, rgb)
    print(f"Fused {xyz.shape[0]} points from {len(views)} views -> {outfile}")
    return args
