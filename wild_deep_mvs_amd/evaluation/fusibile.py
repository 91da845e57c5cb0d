"""Depth-map fusion on MI355X -- drop-in for ``evaluation/fusibile.py`` of fdarmon/wild_deep_mvs.

The reference converts each view's masked depth map to gipuma files and runs the external CUDA-only ``fusibile`` binary
(``evaluation/fusibile.py:162-221``), which does not run on AMD GPUs.  Here the same step is ``pscv_fuse_depth_pass``, one HIP
launch sequence per view (INTEGRATION.md section 2d states the rule; it restates fusibile's consistency fusion as the reference
configures it -- normal test off, depth range (0.001, 100000), ``disp_thresh`` and ``num_consistent`` from the command line -- and
has not been compared with the binary's output).

``run(dataloader, args)`` keeps the reference's interface and writes the file its metrics step reads,
``<data_path>/Points/<model>_<nviews>/<model>_<nviews><scene>.ply``; ``fuse_depth_maps`` is the step as a function from tensors to a
point cloud.

With ``args.fusion_normals = "depth"`` every point also carries the world normal of the pixel that emitted it, estimated from
its view's masked depth map (``ops.depth_normals``, ``ops.point_world_normals``), and the file has
COLMAP's fused layout (``x y z nx ny nz red green blue``), which ``evaluation/metrics.py`` reads by property name like the plain
one.  Points, colours and their order are those of the default run.
"""
from __future__ import annotations

from pathlib import Path
from typing import Sequence

import numpy as np
import torch
from PIL import Image

from .. import ops
from ..utils.point_cloud import write_colmap_point_cloud, write_point_cloud
from .filtering import depth_folder_name

DEPTH_MIN, DEPTH_MAX = 0.001, 100000.0       # fusibile.py:165-166


def fuse_depth_maps(depths: Sequence, images: Sequence, K, R, t, *, disp_thresh: float = 0.01, num_consistent: int = 3,
                    depth_min: float = DEPTH_MIN, depth_max: float = DEPTH_MAX, device="cuda", normal_options=None):
    """depths N x [h_v,w_v] (masked pixels 0), images N x uint8 [h_v,w_v,3], K,R [N,3,3], t [N,3,1] (intrinsics at each depth
    map's resolution; tensors or numpy arrays) -> (xyz fp32 [M,3], rgb uint8 [M,3], view int32 [M]) on ``device``.  With
    ``normal_options`` (a dict of ``ops.depth_normals`` keywords, possibly empty) a fourth result, normal fp32 [M,3]: the world
    normal of each point's emitting pixel from its view's depth map; the first three are the same either way."""
    tens = lambda a: torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a)
    cams = ops.geo_filter_cams(tens(K), tens(R), tens(t)).to(device)
    d = [tens(x).to(device=device, dtype=torch.float32) for x in depths]
    c = [tens(x).to(device=device, dtype=torch.uint8) for x in images]
    kw = dict(disp_thresh=disp_thresh, num_consistent=num_consistent, depth_min=depth_min, depth_max=depth_max)
    if normal_options is None:
        return ops.fuse_depth_maps(d, c, cams, **kw)
    xyz, rgb, view, pixel = ops.fuse_depth_maps(d, c, cams, want_pixel=True, **kw)
    return xyz, rgb, view, ops.point_world_normals(view, pixel, ops.depth_normals(d, cams, **normal_options), cams)


def get_mask(args, filename, prob, geo_mask=None):
    """Invalid pixels of one depth map (``evaluation/pipeline_utils.py:88-109``): probability below ``args.prob_threshold`` (in
    every channel of a multi-channel map), or outside the geometric filter's ``geo_mask`` when ``args.filter`` is set."""
    invalid = (prob < args.prob_threshold).all(axis=0) if prob.ndim > 2 else prob < args.prob_threshold
    if args.filter:
        if geo_mask is None:
            geo_mask = np.load(Path(args.data_path) / "IntRes" / "geometric_filtering" / depth_folder_name(args) / str(args.scene)
                               / f"{filename}_out.npz")["geo_mask"]
        invalid = invalid | ~geo_mask
    return invalid


NORMAL_SOURCES = ("constant", "depth")


def normal_source(args):
    """``args.fusion_normals`` (absent = "constant"), checked: "depth" estimates the network path's normal maps from its depth maps
    and does not go with ``args.colmap``, whose PatchMatch brings its own."""
    mode = getattr(args, "fusion_normals", "constant")
    if mode not in NORMAL_SOURCES:
        raise ValueError(f"fusion_normals must be one of {NORMAL_SOURCES}, got {mode!r}")
    if mode == "depth" and getattr(args, "colmap", False):
        raise ValueError("fusion_normals 'depth' is for the network path: under args.colmap the fusion reads PatchMatch's own normal maps")
    return mode


def depth_normal_options(args):
    """The keyword arguments of ``ops.depth_normals`` from ``args.fusion_normal_radius``, ``fusion_normal_gate`` and
    ``fusion_normal_support`` (each absent = the default of ``ops.depth_normals``)."""
    names = (("radius", "fusion_normal_radius"), ("rel_gate", "fusion_normal_gate"), ("min_support", "fusion_normal_support"))
    return {kw: getattr(args, name) for kw, name in names if getattr(args, name, None) is not None}


def view_colors(img: torch.Tensor, downscale: int) -> np.ndarray:
    """[3,h,w] image in [0,1] -> uint8 [h//downscale, w//downscale, 3] as the reference writes its gipuma images: x 255 truncated
    to a byte (ToPILImage), then a LANCZOS resize (fusibile.py:125)."""
    h, w = img.shape[1:]
    arr = img.detach().cpu().mul(255).byte().permute(1, 2, 0).numpy()
    pil = Image.fromarray(np.ascontiguousarray(arr)).resize((w // downscale, h // downscale), resample=Image.LANCZOS)
    return np.array(pil)


def masked_view(args, batch, depth_folder):
    """(depth with invalid pixels at 0, colours, K, R, t) of a batch's view 0, as mvsnet_to_gipuma prepares it (fusibile.py:104-157)."""
    filename = batch["filename"][0]
    img = batch["imgs"][0, 0]
    h, w = img.shape[1:]
    K = batch["K"][0, 0].clone().to(torch.float32)
    K[:2] /= args.downscale
    npz = np.load(depth_folder / f"{filename}_out.npz")
    depth, prob = np.array(npz["depthmap"], dtype=np.float32), npz["probability"]
    if args.colmap:                                   # crop like the image dataloader
        depth, prob = depth[:h, :w], prob[..., :h, :w]
    degenerate = "degenerate" in batch and bool(torch.as_tensor(batch["degenerate"]).any())
    invalid = np.ones(depth.shape, dtype=bool) if degenerate else get_mask(args, filename, prob)
    depth[invalid] = 0
    colors = view_colors(img, args.downscale)
    if colors.shape[:2] != depth.shape:
        raise ValueError(f"fusion: view {filename}: image of {colors.shape[1]}x{colors.shape[0]} after the 1/{args.downscale} resize "
                         f"does not match its depth map of {depth.shape[1]}x{depth.shape[0]}")
    return depth, colors, K, batch["R"][0, 0].to(torch.float32), batch["t"][0, 0].to(torch.float32)


def run(dataloader, args):
    with_normals = normal_source(args) == "depth"
    folder_name = depth_folder_name(args)
    out_path = Path(args.data_path) / "Points" / folder_name
    outfile = out_path / f"{folder_name}{args.scene}.ply"
    if outfile.exists() and not args.override:
        print("Point cloud fusion already computed")
        return
    depth_folder = Path(args.data_path) / "IntRes" / "depthmaps" / folder_name / str(args.scene)
    views = [masked_view(args, batch, depth_folder) for batch in dataloader]
    depths, colors, K, R, t = zip(*views)
    with torch.no_grad():
        xyz, rgb, _, *normal = fuse_depth_maps(depths, colors, torch.stack(K), torch.stack(R), torch.stack(t),
                                               disp_thresh=args.fusion_depth_threshold, num_consistent=args.fusion_num_consistent,
                                               normal_options=depth_normal_options(args) if with_normals else None)
    out_path.mkdir(parents=True, exist_ok=True)
    if with_normals:
        write_colmap_point_cloud(outfile, xyz, normal[0], rgb)
    else:
        write_point_cloud(outfile, xyz.cpu().numpy(), rgb.cpu().numpy())
    print(f"Fused {xyz.shape[0]} points from {len(views)} views -> {outfile}")
    return args
