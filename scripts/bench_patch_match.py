#!/usr/bin/env python3
"""Time ops.patch_match / ops.patch_match_filter (csrc/patch_match.hip) on one reference view of make_patch_match_scene: 5 views
at 300 x 400, 10 at 600 x 800 and 20 at 1200 x 1600 (S = V - 1 sources, 8 iterations per pass).  The scene is rendered at a
quarter of the size and upsampled x4 (intrinsics scaled), which keeps the setup short.  Device events around each pass after a
warm-up, median of 5.  Reports ms per iteration per view for the photometric and the geometric pass, the filter's ms, and the
tap rate from shapes: h w x 11 candidates x S x taps per iteration.  One JSON line per case.
Usage:  python scripts/bench_patch_match.py [--reps 5] [--cases 5x300x400,...]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from wild_deep_mvs_amd import ops, synthetic  # noqa: E402

CASES = [("5x300x400", 5, 300, 400), ("10x600x800", 10, 600, 800), ("20x1200x1600", 20, 1200, 1600)]
ITERS = 8


def _timed(fn, reps):
    fn()
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
    ap.add_argument("--cases", default=",".join(c[0] for c in CASES))
    a = ap.parse_args()
    for name, V, H, W in CASES:
        if name not in a.cases.split(","):
            continue
        sc = synthetic.make_patch_match_scene(V, H // 4, W // 4, seed=0)
        imgs = F.interpolate(sc["imgs"], size=(H, W), mode="bilinear", align_corners=False).clamp(0, 1)
        K = sc["K"].clone()
        K[:, :2] *= 4.0
        g = [ops.grey_image(im.cuda()) for im in imgs]
        cams = ops.geo_filter_cams(K, sc["R"], sc["t"]).cuda()
        src = sc["src"][0]
        cv = cams[[0] + src].contiguous()
        srcs = [g[s] for s in src]
        dmin, dmax = float(sc["depth_min"][0]), float(sc["depth_max"][0])
        photo, ms_p = _timed(lambda: ops.patch_match(g[0], srcs, cv, dmin, dmax, num_iterations=ITERS), a.reps)
        # the sources' photometric maps: the reference's own map reused (timing only; the work per tap does not depend on it)
        sd = [torch.full((H, W), float(sc["depth"][s].mean()), device="cuda") for s in src]
        _, ms_g = _timed(lambda: ops.patch_match(g[0], srcs, cv, dmin, dmax, num_iterations=ITERS, src_depths=sd, state=photo), a.reps)
        _, ms_f = _timed(lambda: ops.patch_match_filter(photo, g[0], srcs, cv, sd), a.reps)
        S = len(src)
        taps = H * W * 11 * S * 121
        mp, mg = float(np.median(ms_p)) / ITERS, float(np.median(ms_g)) / ITERS
        print(json.dumps({"case": name, "views": V, "sources": S, "h": H, "w": W, "iterations": ITERS,
                          "photometric_ms_per_iter": round(mp, 3), "geometric_ms_per_iter": round(mg, 3),
                          "filter_ms": round(float(np.median(ms_f)), 3), "photometric_gtaps_per_s": round(taps / mp * 1e-6, 1),
                          "photometric_ms_all": [round(x, 2) for x in ms_p]}), flush=True)


if __name__ == "__main__":
    main()
