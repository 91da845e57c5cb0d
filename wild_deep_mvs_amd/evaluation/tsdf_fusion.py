"""TSDF fusion and meshing on MI355X: the surface at the end of the reconstruction pipeline.

The reference (fdarmon/wild_deep_mvs) ends at a fused point cloud and has no counterpart of this step.  The masked depth maps
and colours that ``evaluation/fusibile.py`` prepares for the point-cloud fusion are integrated into a dense truncated signed
distance volume (``ops.tsdf_integrate``) whose zero level set is extracted by marching tetrahedra (``ops.tsdf_extract``).
With ``layout="bricks"`` (``args.tsdf_layout``) the volume is a pool of 8 x 8 x 8 bricks allocated only near the surface
(``ops.tsdf_brick_*``, section 2q): the same mesh from a fraction of the memory, on lattices the dense layout refuses.

``fuse_tsdf_mesh`` is the step as a function from tensors to a mesh; ``run(dataloader, args)`` has the interface of the other
evaluation steps and writes ``<data_path>/Meshes/<model>_<nviews>/<model>_<nviews><scene>.ply``.  It is opt-in: nothing else
calls it, and no other step's output changes.

``clean_mesh`` is the optional step between extraction and the file: small connected components
(the closed blobs that depth outliers leave in front of and behind the surface), degenerate faces and unused vertices are
removed, and area-weighted vertex normals are added.  ``run`` applies it only when one of its arguments is set; with none
set it writes the same bytes as before.
"""
from __future__ import annotations

import math
from pathlib import Path
from typing import Sequence

import numpy as np
import torch

from .. import ops
from ..utils.point_cloud import write_mesh, write_point_cloud
from .filtering import depth_folder_name
from .fusibile import masked_view


def _valid(d: torch.Tensor) -> torch.Tensor:
    return (d > 0) & (d <= torch.finfo(torch.float32).max)


def default_voxel(depths: Sequence[torch.Tensor], K: torch.Tensor) -> float:
    """Twice the median over the views of the per-view median of d / K[0,0] over the valid pixels: about two pixel footprints.
    Views without a valid pixel do not count; none at all is a ValueError."""
    per_view = [(d[_valid(d)] / k[0, 0]).median() for d, k in zip(depths, K) if bool(_valid(d).any())]
    if not per_view:
        raise ValueError("fuse_tsdf_mesh: no depth map has a valid pixel; pass voxel and bounds")
    return 2.0 * float(torch.stack(per_view).median())


def world_bounds(depths: Sequence[torch.Tensor], K: torch.Tensor, R: torch.Tensor, t: torch.Tensor):
    """(lo, hi): the per-axis extremes (float64 tuples) of R^T (d K^-1 (x, y, 1) - t) over the valid pixels of all views, unprojected
    with torch on the depth maps' device in fp64."""
    lo, hi = [], []
    for d, k, r, tt in zip(depths, K, R, t):
        ok = _valid(d)
        if not bool(ok.any()):
            continue
        ys, xs = torch.nonzero(ok, as_tuple=True)
        dd = d[ok].to(torch.float64)
        pix = torch.stack((xs.to(torch.float64) * dd, ys.to(torch.float64) * dd, dd), dim=0)
        cam = torch.inverse(k.to(device=d.device, dtype=torch.float64)) @ pix - tt.to(device=d.device, dtype=torch.float64).reshape(3, 1)
        X = r.to(device=d.device, dtype=torch.float64).t() @ cam
        lo.append(X.amin(dim=1))
        hi.append(X.amax(dim=1))
    if not lo:
        raise ValueError("fuse_tsdf_mesh: no depth map has a valid pixel; pass voxel and bounds")
    return tuple(torch.stack(lo).amin(dim=0).tolist()), tuple(torch.stack(hi).amax(dim=0).tolist())


def grid_dims(lo, hi, voxel: float):
    """Lattice points per axis so that lo + (n - 1) voxel >= hi."""
    return tuple(int(math.ceil((b - a) / voxel)) + 1 for a, b in zip(lo, hi))


def fuse_tsdf_mesh(depths: Sequence, images: Sequence, K, R, t, *, voxel=None, trunc_voxels: float = 3, min_weight: int = 1,
                   bounds=None, max_voxels: int = 2 ** 31 - 1, device="cuda", layout: str = "dense", max_bricks=None):
    """depths N x [h_v,w_v] (masked pixels 0), images N x uint8 [h_v,w_v,3], K,R [N,3,3], t [N,3,1] (intrinsics at each depth map's
    resolution; tensors or numpy arrays) -> (xyz fp32 [V,3], rgb uint8 [V,3], faces int32 [F,3]) on ``device``.  ``voxel`` None =
    ``default_voxel``; the truncation is ``trunc_voxels`` voxels; ``bounds`` = ((x0,y0,z0), (x1,y1,z1)) or None = the extent of
    the unprojected valid pixels padded by the truncation.  A grid of more than ``max_voxels`` lattice points is a ValueError.
    ``device`` is where the inputs are moved to and the volume lives, as in ``fusibile.fuse_depth_maps``; the ops run on a GPU only.
    ``layout`` "bricks" stores the same lattice (the same lo, dims and voxel) as a pool of 8 x 8 x 8 bricks allocated only near the
    surface: the mesh holds the same vertices, colours and triangles bit for bit, in brick order.
    ``max_voxels`` does not apply to it; more than ``max_bricks`` (None: 2^22 - 1) bricks is a ValueError."""
    tens = lambda a: torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a)
    K, R, t = tens(K).to(torch.float32), tens(R).to(torch.float32), tens(t).to(torch.float32)
    d = [tens(x).to(device=device, dtype=torch.float32) for x in depths]
    c = [tens(x).to(device=device, dtype=torch.uint8) for x in images]
    if layout not in ("dense", "bricks"):
        raise ValueError(f"fuse_tsdf_mesh: layout must be 'dense' or 'bricks', got {layout!r}")
    if not (float(trunc_voxels) > 0.0 and math.isfinite(float(trunc_voxels))):
        raise ValueError(f"fuse_tsdf_mesh: trunc_voxels must be positive and finite, got {trunc_voxels}")
    s = default_voxel(d, K) if voxel is None else float(voxel)
    if not (s > 0.0 and math.isfinite(s)):
        raise ValueError(f"fuse_tsdf_mesh: voxel must be positive and finite, got {voxel}")
    trunc = float(trunc_voxels) * s
    if bounds is None:
        lo, hi = world_bounds(d, K, R, t)
        lo, hi = tuple(v - trunc for v in lo), tuple(v + trunc for v in hi)
    else:
        lo, hi = (tuple(float(v) for v in b) for b in bounds)
        if len(lo) != 3 or len(hi) != 3 or not all(math.isfinite(a) and math.isfinite(b) and a <= b for a, b in zip(lo, hi)):
            raise ValueError(f"fuse_tsdf_mesh: bounds must be ((x0,y0,z0), (x1,y1,z1)) with finite lo <= hi, got {bounds!r}")
    dims = grid_dims(lo, hi, s)
    if layout == "bricks":
        cams = ops.geo_filter_cams(K, R, t).to(device)
        masks = ops.tsdf_brick_probe(d, cams, dims, origin=lo, voxel=s, trunc=trunc)
        bricks = ops.tsdf_bricks(masks, dims, max_bricks)
        ops.tsdf_brick_integrate(bricks, d, c, cams, origin=lo, voxel=s, trunc=trunc)
        return ops.tsdf_brick_extract(bricks, origin=lo, voxel=s, min_weight=min_weight)
    if dims[0] * dims[1] * dims[2] > min(int(max_voxels), ops.TSDF_MAX_VOXELS):
        raise ValueError(f"fuse_tsdf_mesh: the grid of {dims[0]} x {dims[1]} x {dims[2]} voxels of {s:g} exceeds max_voxels = "
                         f"{max_voxels}: pass `bounds` or a larger `voxel`")
    cams = ops.geo_filter_cams(K, R, t).to(device)
    state = ops.tsdf_volume(dims, device)
    ops.tsdf_integrate(state, d, c, cams, origin=lo, voxel=s, trunc=trunc)
    return ops.tsdf_extract(state, origin=lo, voxel=s, min_weight=min_weight)


def tsdf_options(args):
    """The keyword arguments of ``fuse_tsdf_mesh`` from ``args.tsdf_voxel``, ``tsdf_trunc_voxels``, ``tsdf_min_weight``,
    ``tsdf_bounds``, ``tsdf_layout`` and ``tsdf_max_bricks`` (each absent or None = the default of ``fuse_tsdf_mesh``)."""
    names = (("voxel", "tsdf_voxel"), ("trunc_voxels", "tsdf_trunc_voxels"), ("min_weight", "tsdf_min_weight"), ("bounds", "tsdf_bounds"),
             ("layout", "tsdf_layout"), ("max_bricks", "tsdf_max_bricks"))
    return {kw: getattr(args, name) for kw, name in names if getattr(args, name, None) is not None}


def clean_mesh(xyz, rgb, faces, *, min_component_faces: int = 0, min_component_fraction: float = 0.0, keep_largest: int = 0,
               drop_degenerate: bool = False, vertex_normals: bool = False):
    """(xyz, rgb, faces) of ``fuse_tsdf_mesh`` -> (xyz, rgb, faces, normals): ``ops.mesh_clean`` with the four choices (with all of
    them at their defaults it only drops the vertices no face uses), then, with ``vertex_normals``, ``ops.mesh_vertex_normals`` of
    the cleaned mesh (fp32 [V,3], pointing to free space like the faces); normals is None otherwise."""
    xyz, rgb, faces = ops.mesh_clean(xyz, rgb, faces, min_component_faces=min_component_faces,
                                     min_component_fraction=min_component_fraction, keep_largest=keep_largest,
                                     drop_degenerate=drop_degenerate)
    return xyz, rgb, faces, (ops.mesh_vertex_normals(xyz, faces) if vertex_normals else None)


def clean_options(args):
    """The keyword arguments of ``clean_mesh`` from ``args.tsdf_min_component_faces``, ``tsdf_min_component_fraction``,
    ``tsdf_keep_largest``, ``tsdf_drop_degenerate`` and ``tsdf_vertex_normals`` (each absent, None or False = off).  Empty = ``run``
    writes the extracted mesh as it is; any argument set, a 0 included, runs ``clean_mesh``, which at least drops unused vertices."""
    names = (("min_component_faces", "tsdf_min_component_faces"), ("min_component_fraction", "tsdf_min_component_fraction"),
             ("keep_largest", "tsdf_keep_largest"), ("drop_degenerate", "tsdf_drop_degenerate"), ("vertex_normals", "tsdf_vertex_normals"))
    values = ((kw, getattr(args, name, None)) for kw, name in names)
    return {kw: v for kw, v in values if v is not None and v is not False}


def run(dataloader, args):
    folder_name = depth_folder_name(args)
    out_path = Path(args.data_path) / "Meshes" / folder_name
    outfile = out_path / f"{folder_name}{args.scene}.ply"
    if outfile.exists() and not args.override:
        print("TSDF mesh already computed")
        return
    options, cleaning = tsdf_options(args), clean_options(args)
    depth_folder = Path(args.data_path) / "IntRes" / "depthmaps" / folder_name / str(args.scene)
    views = [masked_view(args, batch, depth_folder) for batch in dataloader]
    depths, colors, K, R, t = zip(*views)
    with torch.no_grad():
        xyz, rgb, faces = fuse_tsdf_mesh(depths, colors, torch.stack(K), torch.stack(R), torch.stack(t), **options)
        normals = None
        if cleaning:
            xyz, rgb, faces, normals = clean_mesh(xyz, rgb, faces, **cleaning)
    out_path.mkdir(parents=True, exist_ok=True)
    if normals is None:
        write_mesh(outfile, xyz, rgb, faces)
    else:
        write_mesh(outfile, xyz, rgb, faces, normals)
    if getattr(args, "tsdf_write_points", False):                  # the vertices as the cloud evaluation/metrics.py reads
        points_path = Path(args.data_path) / "Points" / folder_name
        points_path.mkdir(parents=True, exist_ok=True)
        write_point_cloud(points_path / f"{folder_name}{args.scene}.ply", xyz, rgb)
    print(f"Meshed {xyz.shape[0]} vertices and {faces.shape[0]} faces from {len(views)} views -> {outfile}")
    return args
