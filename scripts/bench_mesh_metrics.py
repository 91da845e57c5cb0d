#!/usr/bin/env python3
"""Time the mesh metrics (csrc/mesh_metrics.hip; ops.mesh_sample / ops.mesh_dist) on the mesh that evaluation.tsdf_fusion.
fuse_tsdf_mesh extracts from the default scene of scripts/bench_tsdf.py: 49 views of 1200 x 1600 in a grid of 640 x 512 x 256
(voxel 0.01; about 1.23 M vertices, 2.46 M faces).  Device events around a window of calls sized to last about 20 ms, after a
warm-up, median of --reps windows (bench_tsdf.window_ms); every figure is a whole ops call: torch plumbing, allocation, the grid
builds and the host reads included.  One JSON line with
  mesh_sample        ops.mesh_sample at --spacing-voxels (default 0.5) voxels, with the faces;
  mesh_dist_near     ops.mesh_dist for queries within two voxels of the surface (the samples, each moved by up to two voxels),
                     maxdist = --maxdist-voxels (default 20) voxels;
  mesh_dist_mixed    the same with --far-share (default 0.25) of the queries moved beyond maxdist (1.5 to 3 maxdist along z);
  kernels_ms         the launches of one mesh_dist_near call, by name (ops.EventTimer): the two grid builds and the search;
  nn_dist            for scale: the existing ops.nn_dist from the same queries to the sampled cloud (near, mixed);
  host               for scale: scipy.spatial.cKDTree built on the samples and queried with --host-queries of the near queries
                     (distance_upper_bound = maxdist), or, without SciPy, the numpy rule of tests/_mesh_metrics_ref.py on
                     --host-queries queries against the first --host-faces faces; timed once with a host clock.
Usage:  python scripts/bench_mesh_metrics.py [--reps 7] [--case 49x1200x1600:640x512x256]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_tsdf import TRUNC_VOXELS, make_views, window_ms  # noqa: E402
from wild_deep_mvs_amd import ops  # noqa: E402
from wild_deep_mvs_amd.evaluation.tsdf_fusion import fuse_tsdf_mesh  # noqa: E402


def extract_mesh(V, h, w, dims):
    """The mesh of bench_tsdf's scene through fuse_tsdf_mesh, on bench_tsdf's lattice -> (xyz, rgb, faces, voxel)."""
    depths, colors, cams = make_views(V, h, w)
    voxel = 6.4 / dims[0]
    lo = (-0.5 * voxel * (dims[0] - 1), -0.5 * voxel * (dims[1] - 1), 4.0 - 0.5 * voxel * (dims[2] - 1))
    hi = tuple(o + voxel * (n - 1) for o, n in zip(lo, dims))
    c = cams.cpu()
    K, R, t = c[:, 0:9].reshape(V, 3, 3), c[:, 18:27].reshape(V, 3, 3), c[:, 27:30].reshape(V, 3, 1)
    xyz, rgb, faces = fuse_tsdf_mesh(depths, colors, K, R, t, voxel=voxel, trunc_voxels=TRUNC_VOXELS, bounds=(lo, hi))
    return xyz, rgb, faces, voxel


def host_scale(samples, near, maxdist, xyz, faces, n_queries, n_faces):
    q = near[:n_queries].cpu().numpy()
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        from tests import _mesh_metrics_ref as R
        x, f = xyz.cpu().numpy(), faces[:n_faces].cpu().numpy()
        t0 = time.perf_counter()
        R.dist(q, x, f, maxdist)
        return {"what": "numpy rule", "queries": len(q), "faces": len(f), "ms": round((time.perf_counter() - t0) * 1e3, 1)}
    pts = samples.cpu().numpy()
    t0 = time.perf_counter()
    tree = cKDTree(pts)
    t1 = time.perf_counter()
    tree.query(q, k=1, distance_upper_bound=maxdist)
    t2 = time.perf_counter()
    return {"what": "scipy cKDTree on the samples", "points": len(pts), "queries": len(q), "build_ms": round((t1 - t0) * 1e3, 1),
            "query_ms": round((t2 - t1) * 1e3, 1), "query_us_per_point": round((t2 - t1) * 1e6 / max(len(q), 1), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--case", default="49x1200x1600:640x512x256")
    ap.add_argument("--spacing-voxels", type=float, default=0.5)
    ap.add_argument("--maxdist-voxels", type=float, default=20.0)
    ap.add_argument("--far-share", type=float, default=0.25)
    ap.add_argument("--host-queries", type=int, default=200_000)
    ap.add_argument("--host-faces", type=int, default=20_000)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_metrics: needs the GPU (no time is reported without one)")
    views, grid = a.case.split(":")
    V, h, w = (int(x) for x in views.split("x"))
    xyz, rgb, faces, voxel = extract_mesh(V, h, w, tuple(int(x) for x in grid.split("x")))
    del rgb
    torch.cuda.empty_cache()
    spacing, maxdist = a.spacing_voxels * voxel, a.maxdist_voxels * voxel
    s_ms, s_all, s_inner = window_ms(lambda: ops.mesh_sample(xyz, faces, spacing, return_faces=True), a.reps)
    samples, _ = ops.mesh_sample(xyz, faces, spacing, return_faces=True)
    m = int(samples.shape[0])
    g = torch.Generator(device="cuda").manual_seed(1)
    step = torch.randn((m, 3), device="cuda", generator=g)
    step = step / step.norm(dim=1, keepdim=True) * (2.0 * voxel * torch.rand((m, 1), device="cuda", generator=g))
    near = (samples + step).contiguous()
    mixed = near.clone()
    n_far = int(a.far_share * m)
    pick = torch.randperm(m, device="cuda", generator=g)[:n_far]
    mixed[pick, 2] += maxdist * (1.5 + 1.5 * torch.rand(n_far, device="cuda", generator=g)) * (
        torch.randint(0, 2, (n_far,), device="cuda", generator=g) * 2 - 1)
    out = {"case": a.case, "voxel": voxel, "vertices": int(xyz.shape[0]), "faces": int(faces.shape[0]), "spacing": spacing,
           "samples": m, "maxdist": maxdist, "queries": m, "far_share": a.far_share,
           "mesh_sample_ms": round(s_ms, 4), "mesh_sample_all": s_all, "calls_per_window": s_inner}
    for name, q in (("near", near), ("mixed", mixed)):
        ms, all_ms, inner = window_ms(lambda: ops.mesh_dist(q, xyz, faces, maxdist, return_faces=True), a.reps)
        d = ops.mesh_dist(q, xyz, faces, maxdist)
        out[f"mesh_dist_{name}_ms"] = round(ms, 4)
        out[f"mesh_dist_{name}_all"] = all_ms
        out[f"mesh_dist_{name}_ns_per_query"] = round(ms * 1e6 / m, 2)
        out[f"mesh_dist_{name}_inf_share"] = round(float(torch.isinf(d).double().mean()), 4)
        nn_ms, _, _ = window_ms(lambda: ops.nn_dist(q, samples, maxdist), a.reps)
        out[f"nn_dist_{name}_ms"] = round(nn_ms, 4)
    with ops.EventTimer() as tm:
        ops.mesh_dist(near, xyz, faces, maxdist, return_faces=True)
    out["kernels_ms"] = {k: [n, round(ms, 4)] for k, (n, ms) in tm.summary().items()}
    out["host"] = host_scale(samples, near, maxdist, xyz, faces, a.host_queries, a.host_faces)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
