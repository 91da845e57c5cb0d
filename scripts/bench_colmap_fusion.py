#!/usr/bin/env python3
"""Time ops.colmap_fuse (csrc/colmap_fusion.hip) on synthetic YFCC-like scenes: 10 and 20 views at 1/4 resolution (300 x 400)
and 49 views at 1200 x 1600.  Device events around the whole run after warm-up, median of 5.  Prints one JSON line per case.
With --normals the same three cases also run with normal maps and max_normal_error = 10 degrees (pscv_colmap_fuse_pass_normals):
the ragged scenes have no surface normals of their own, so every view gets the plane's world normal (0.10, -0.06, 1) / |.|, facing
the cameras and turned into the view's frame, with a seeded Gaussian jitter of 2.5 degrees per tangent axis;
the line then carries the time next to the normal-free time of the same run and their ratio.
Usage:  python scripts/bench_colmap_fusion.py [--reps 5] [--normals]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from wild_deep_mvs_amd import ops, synthetic  # noqa: E402

CASES = [("10x300x400", 10, 300, 400), ("20x300x400", 20, 300, 400), ("49x1200x1600", 49, 1200, 1600)]


def plane_normals(sc, seed=0, jitter_deg=2.5):
    """One fp32 [h_v, w_v, 3] camera-frame normal map per view of a make_yfcc_fusion_scene scene: its plane's normal, facing the
    cameras, with a Gaussian tangent jitter; 0 where the depth is masked."""
    rng = np.random.default_rng(seed)
    n = np.array([0.10, -0.06, 1.0])
    n = -n / np.linalg.norm(n)
    out = []
    for d, R in zip(sc["depths"], sc["R"].numpy().astype(np.float64)):
        g = rng.standard_normal(tuple(d.shape) + (3,))
        w = n + np.radians(jitter_deg) * (g - (g @ n)[..., None] * n)
        w /= np.linalg.norm(w, axis=-1, keepdims=True)
        m = w @ R.T                                                   # R w: world -> camera frame
        m[d.numpy() == 0] = 0.0
        out.append(torch.from_numpy(m.astype(np.float32)).contiguous())
    return out


def timed(fn, reps):
    out = fn()                                                        # warm-up
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return out, ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--normals", action="store_true", help="also time the run with normal maps (max_normal_error = 10 degrees)")
    ap.add_argument("--cases", default=",".join(c[0] for c in CASES))
    a = ap.parse_args()
    for name, V, H, W in CASES:
        if name not in a.cases.split(","):
            continue
        sc = synthetic.make_yfcc_fusion_scene(V, H, W, seed=0)
        cams = ops.geo_filter_cams(sc["K"], sc["R"], sc["t"]).cuda()
        depths = [d.cuda() for d in sc["depths"]]
        colors = [c.cuda() for c in sc["colors"]]
        kw = dict(max_depth_error=0.01, max_reproj_error=1.0, min_num_pixels=3)
        out, ms = timed(lambda: ops.colmap_fuse(depths, colors, cams, sc["overlap"], **kw), a.reps)
        line = {"case": name, "views": V, "h": H, "w": W, "points": int(out[0].shape[0]),
                "ms_median": float(np.median(ms)), "ms_all": [round(x, 3) for x in ms]}
        if a.normals:
            normals = [n.cuda() for n in plane_normals(sc)]
            out, msn = timed(lambda: ops.colmap_fuse(depths, colors, cams, sc["overlap"], normals=normals, max_normal_error=10.0, **kw),
                             a.reps)
            line.update({"normals_points": int(out[0].shape[0]), "normals_ms_median": float(np.median(msn)),
                         "normals_ms_all": [round(x, 3) for x in msn], "normals_over_plain": float(np.median(msn) / np.median(ms))})
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
