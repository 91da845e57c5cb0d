#!/usr/bin/env python3
"""Time ops.colmap_fuse (csrc/colmap_fusion.hip) on synthetic YFCC-like scenes: 10 and 20 views at 1/4 resolution (300 x 400)
and 49 views at 1200 x 1600.  Device events around the whole run after warm-up, median of 5.  Prints one JSON line per case.
Usage:  python scripts/bench_colmap_fusion.py [--reps 5]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from wild_deep_mvs_amd import ops, synthetic  # noqa: E402

CASES = [("10x300x400", 10, 300, 400), ("20x300x400", 20, 300, 400), ("49x1200x1600", 49, 1200, 1600)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
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
        out = ops.colmap_fuse(depths, colors, cams, sc["overlap"], **kw)          # warm-up
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = ops.colmap_fuse(depths, colors, cams, sc["overlap"], **kw)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        print(json.dumps({"case": name, "views": V, "h": H, "w": W, "points": int(out[0].shape[0]),
                          "ms_median": float(np.median(ms)), "ms_all": [round(x, 3) for x in ms]}), flush=True)


if __name__ == "__main__":
    main()
