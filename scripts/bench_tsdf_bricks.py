#!/usr/bin/env python3
"""Time the brick layout of the TSDF volume (csrc/tsdf_bricks.hip) beside the dense one, with the scene
and the method of scripts/bench_tsdf.py: device events around a window of calls sized to last about 20 ms, after a warm-up, median
of --reps windows.  One JSON line per case with
  bricks.touched / allocated / directory   bricks that hold a touched point, bricks of the pool, bricks of the lattice,
  bricks.state_bytes, dense_state_bytes    n 512 x 24 B against 24 B per lattice point (the directory and brick_ids are counted),
  bricks.ms_probe, ms_allocate, ms_integrate, ms_extract   ops.tsdf_brick_probe, ops.tsdf_bricks, ops.tsdf_brick_integrate and
                                           ops.tsdf_brick_extract as a user calls them; ms_whole: the four in a row,
  dense.ms_integrate, ms_extract, ms_whole the same for ops.tsdf_volume + tsdf_integrate + tsdf_extract, when the dense layout takes
                                           the lattice (nx ny nz < 2^31 and the state fits --dense-max-gb); else "refused",
  same_mesh                                the two meshes hold the same vertex rows and the same faces as sorted multisets.
Usage:  python scripts/bench_tsdf_bricks.py [--reps 7] [--cases 49x1200x1600:640x512x256,49x1200x1600:2560x2048x1024]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from bench_tsdf import TRUNC_VOXELS, make_views, window_ms  # noqa: E402
from wild_deep_mvs_amd import ops  # noqa: E402


def rows(xyz, rgb, faces=None):
    """Vertex rows (xyz bits, rgb) or face rows (three vertex rows in stored order), sorted."""
    v = torch.cat((xyz.contiguous().view(torch.int32).long(), rgb.long()), dim=1)
    r = v if faces is None else v[faces.long()].reshape(faces.shape[0], -1)
    return torch.unique(r, dim=0, return_counts=True)


def same(a, b):
    return all(x.shape == y.shape and bool((x == y).all()) for x, y in zip(a, b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cases", default="49x1200x1600:640x512x256,49x1200x1600:2560x2048x1024")
    ap.add_argument("--dense-max-gb", type=float, default=64.0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tsdf_bricks: needs the GPU (no time is reported without one)")
    for case in a.cases.split(","):
        views, grid = case.split(":")
        V, h, w = (int(x) for x in views.split("x"))
        dims = tuple(int(x) for x in grid.split("x"))
        nvox = dims[0] * dims[1] * dims[2]
        depths, colors, cams = make_views(V, h, w)
        packed = [ops.pack_rgba8(c) for c in colors]
        voxel = 6.4 / dims[0]                                             # the grid of bench_tsdf.py: 6.4 wide, centred on the plane
        origin = (-0.5 * voxel * (dims[0] - 1), -0.5 * voxel * (dims[1] - 1), 4.0 - 0.5 * voxel * (dims[2] - 1))
        kw = dict(origin=origin, voxel=voxel, trunc=TRUNC_VOXELS * voxel)
        ekw = dict(origin=origin, voxel=voxel, min_weight=1)

        masks = ops.tsdf_brick_probe(depths, cams, dims, **kw)
        bricks = ops.tsdf_bricks(masks, dims)
        n = int(bricks.brick_ids.shape[0])

        def integrate_bricks():
            bricks.views = 0                                              # (timing only: the view limit guards real colour sums)
            ops.tsdf_brick_integrate(bricks, depths, packed, cams, **kw)

        def whole_bricks():
            b = ops.tsdf_bricks(ops.tsdf_brick_probe(depths, cams, dims, **kw), dims)
            ops.tsdf_brick_integrate(b, depths, packed, cams, **kw)
            return ops.tsdf_brick_extract(b, **ekw)
        ms_probe, _, _ = window_ms(lambda: ops.tsdf_brick_probe(depths, cams, dims, **kw), a.reps)
        ms_alloc, _, _ = window_ms(lambda: ops.tsdf_bricks(masks, dims), a.reps)
        ms_int, _, _ = window_ms(integrate_bricks, a.reps)
        ms_whole, _, _ = window_ms(whole_bricks, a.reps)
        mesh_b = whole_bricks()                                           # one clean volume for the extraction and the comparison
        clean = ops.tsdf_bricks(masks, dims)
        ops.tsdf_brick_integrate(clean, depths, packed, cams, **kw)
        ms_ext, _, _ = window_ms(lambda: ops.tsdf_brick_extract(clean, **ekw), a.reps)
        out = {"case": case, "lattice_points": nvox, "voxel": round(voxel, 5),
               "bricks": {"touched": int((masks >> 13 & 1).sum()), "allocated": n, "directory": int(masks.numel()),
                          "state_bytes": n * ops.TSDF_BRICK_BYTES + 4 * int(masks.numel()) + 4 * n, "vertices": int(mesh_b[0].shape[0]),
                          "faces": int(mesh_b[2].shape[0]), "ms_probe": round(ms_probe, 4), "ms_allocate": round(ms_alloc, 4),
                          "ms_integrate": round(ms_int, 4), "ms_extract": round(ms_ext, 4), "ms_whole": round(ms_whole, 4)},
               "dense_state_bytes": 24 * nvox}
        out["bricks"]["state_over_dense"] = round(out["bricks"]["state_bytes"] / out["dense_state_bytes"], 4)
        del clean, bricks
        torch.cuda.empty_cache()
        if nvox <= ops.TSDF_MAX_VOXELS and 24 * nvox <= a.dense_max_gb * 2 ** 30:
            state = ops.tsdf_volume(dims)

            def integrate_dense():
                state.views = 0
                ops.tsdf_integrate(state, depths, packed, cams, **kw)

            def whole_dense():
                s = ops.tsdf_volume(dims)
                ops.tsdf_integrate(s, depths, packed, cams, **kw)
                return ops.tsdf_extract(s, **ekw)
            d_int, _, _ = window_ms(integrate_dense, a.reps)
            d_whole, _, _ = window_ms(whole_dense, a.reps)
            mesh_d = whole_dense()
            state = ops.tsdf_volume(dims)
            ops.tsdf_integrate(state, depths, packed, cams, **kw)
            d_ext, _, _ = window_ms(lambda: ops.tsdf_extract(state, **ekw), a.reps)
            out["dense"] = {"ms_integrate": round(d_int, 4), "ms_extract": round(d_ext, 4), "ms_whole": round(d_whole, 4)}
            out["same_mesh"] = same(rows(*mesh_d[:2]), rows(*mesh_b[:2])) and same(rows(*mesh_d), rows(*mesh_b))
            del state, mesh_d
        else:
            out["dense"] = "refused: " + ("nx ny nz >= 2^31" if nvox > ops.TSDF_MAX_VOXELS else f"{24 * nvox / 2 ** 30:.0f} GiB of state")
        print(json.dumps(out), flush=True)
        del mesh_b, masks, depths, colors, packed
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
