"""PatchMatch stereo on MI355X -- drop-in for ``utils/colmap_utils.py:depthmap_colmap`` of fdarmon/wild_deep_mvs.

The reference runs the external ``colmap image_undistorter`` and ``colmap patch_match_stereo`` binaries
(``utils/colmap_utils.py:282-322``); COLMAP builds its dense stereo only with CUDA.  Here the stereo is ``ops.patch_match`` /
``ops.patch_match_filter`` (HIP, ``csrc/patch_match.hip``).  INTEGRATION.md section 2h states the rule -- COLMAP's photometric
pass, geometric pass and filter, recalled from its defaults and Schoenberger et al. 2016 and not compared with the binary -- and
names its deviations from COLMAP.

``depthmap_colmap(dataloader, args)`` keeps the reference's interface: it returns at once when ``IntRes/colmap_dense/<scene>``
exists, writes COLMAP's workspace maps ``stereo/{depth_maps,normal_maps}/<f>.jpg.{photometric,geometric}.bin`` (``Mat`` layout;
the geometric maps are the filtered ones) and ``IntRes/direct_depthmaps/colmap/<scene>/<f>_out.npz`` (``depthmap`` = the filtered
geometric depth, ``probability`` all ones), the file the rest of the pipeline reads.
"""
from __future__ import annotations

from pathlib import Path

import numpy as np
import torch

from .. import ops
from ..utils.colmap_array import write_array

NUM_ITERATIONS = 8


def _name(x):
    return x[0] if isinstance(x, (list, tuple)) else str(x)


def _view_inputs(batch):
    """(reference grey, source greys, cams [V,30], depth range) of one batch, on the GPU."""
    imgs = batch["imgs"]
    imgs = [im[0] for im in imgs] if isinstance(imgs, (list, tuple)) else list(imgs[0])
    V = len(imgs)
    greys = [ops.grey_image(im.cuda()) for im in imgs]
    K = batch["K"][0].reshape(V, 3, 3).to(torch.float32)
    R = batch["R"][0].reshape(V, 3, 3).to(torch.float32)
    t = batch["t"][0].reshape(V, 3, 1).to(torch.float32)
    cams = ops.geo_filter_cams(K, R, t).cuda()
    return greys[0], greys[1:], cams, (float(batch["depth_min"][0][0]), float(batch["depth_max"][0][0]))


def depthmap_colmap(dataloader, args):
    dense_folder = Path(args.data_path) / "IntRes" / "colmap_dense" / str(args.scene)
    if dense_folder.exists():
        print("Dense colmap already computed")
        return
    depth_dir, normal_dir = dense_folder / "stereo" / "depth_maps", dense_folder / "stereo" / "normal_maps"
    depth_dir.mkdir(parents=True)
    normal_dir.mkdir(parents=True)
    out_dir = Path(args.data_path) / "IntRes" / "direct_depthmaps" / "colmap" / str(args.scene)
    iters = int(getattr(args, "pm_iterations", NUM_ITERATIONS))
    seed = int(getattr(args, "pm_seed", 0))
    photo, views = {}, []
    with torch.no_grad():
        # photometric pass of every view; the states stay on the device for the geometric pass
        for v, b in enumerate(dataloader):
            name = _name(b["filename"])
            ref, srcs, cams, (dmin, dmax) = _view_inputs(b)
            state = ops.patch_match(ref, srcs, cams, dmin, dmax, num_iterations=iters, seed=seed, view=v)
            photo[name] = state
            views.append((v, name, [_name(f) for f in b["src_filenames"]]))
            s = state.cpu().numpy()
            write_array(np.ascontiguousarray(s[..., 0]), depth_dir / f"{name}.jpg.photometric.bin")
            write_array(np.ascontiguousarray(s[..., 1:]), normal_dir / f"{name}.jpg.photometric.bin")
        # geometric pass against the sources' photometric depths, then the filter
        for (v, name, src_names), b in zip(views, dataloader):
            ref, srcs, cams, (dmin, dmax) = _view_inputs(b)
            sd = [photo[n][..., 0].contiguous() if n in photo else torch.zeros_like(s) for n, s in zip(src_names, srcs)]
            state = ops.patch_match(ref, srcs, cams, dmin, dmax, num_iterations=iters, seed=seed, view=v, src_depths=sd,
                                    state=photo[name])
            depth, normal = ops.patch_match_filter(state, ref, srcs, cams, sd)
            d, n = depth.cpu().numpy(), normal.cpu().numpy()
            write_array(d, depth_dir / f"{name}.jpg.geometric.bin")
            write_array(n, normal_dir / f"{name}.jpg.geometric.bin")
            out_dir.mkdir(parents=True, exist_ok=True)
            np.savez(out_dir / f"{name}_out.npz", depthmap=d, probability=np.ones_like(d))
    print(f"PatchMatch stereo of {len(views)} views -> {dense_folder}")
    return args
