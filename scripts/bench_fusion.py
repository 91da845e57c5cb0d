#!/usr/bin/env python3
"""Depth-map fusion (the fusibile step after the geometric filter) at scene size: pscv_fuse_depth_pass over all views on the GPU,
timed with device events after warm-up; the numpy statement of the rule (tests/_fusion_ref.py) timed at a small size on the host
and extrapolated per (pixel, view) test.  Prints one JSON line per size.
Usage: python scripts/bench_fusion.py [--sizes dtu,mvsnet] [--views 49] [--reps 5] [--no-cpu]
  dtu    = 49 views at 1200 x 1600 (DTU, depth maps upsampled to the image size)
  mvsnet = 49 views at 300 x 400 (MVSNet output at 1/4)"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wild_deep_mvs_amd import ops, synthetic  # noqa: E402

SIZES = {"dtu": (1200, 1600), "mvsnet": (300, 400)}
DISP_THRESH, NUM_CONSISTENT = 0.25, 3


def gpu_case(V, H, W, reps):
    sc = synthetic.make_fusion_scene(V, H, W, seed=0)
    d = [x.cuda() for x in sc["depths"]]
    c = [x.cuda() for x in sc["colors"]]
    cams = ops.geo_filter_cams(sc["K"], sc["R"], sc["t"]).cuda()
    run = lambda: ops.fuse_depth_maps(d, c, cams, disp_thresh=DISP_THRESH, num_consistent=NUM_CONSISTENT)
    xyz, _, _ = run()                       # warm-up (also loads the code objects); returns after reading the count
    run()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = run()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    tests = V * (V - 1) * H * W
    ms = sorted(times)[len(times) // 2]
    return {"metric": "depth-map fusion, ms per scene", "value": ms, "unit": "ms",
            "config": {"views": V, "h": H, "w": W, "disp_thresh": DISP_THRESH, "num_consistent": NUM_CONSISTENT},
            "ms_all_reps": [round(t, 3) for t in times], "pixel_view_tests_per_s": tests / (ms * 1e-3),
            "points": int(out[0].shape[0]), "input_pixels": V * H * W}


def cpu_case(V, H, W):
    from tests import _fusion_ref as FR
    sc = synthetic.make_fusion_scene(V, H, W, seed=0)
    cams = ops.geo_filter_cams(sc["K"], sc["R"], sc["t"]).numpy()
    t0 = time.time()
    FR.fuse_all([x.numpy() for x in sc["depths"]], [x.numpy() for x in sc["colors"]], cams, disp_thresh=DISP_THRESH,
                num_consistent=NUM_CONSISTENT)
    dt = time.time() - t0
    return dt, V * (V - 1) * H * W


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="dtu,mvsnet")
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fusion.py measures the GPU kernel: no GPU here")
    cpu = None
    if not a.no_cpu:
        dt, n = cpu_case(a.views, 60, 80)
        cpu = {"measured": f"numpy rule, {a.views} views at 60x80, {dt:.2f} s", "tests_per_s": n / dt}
    for name in a.sizes.split(","):
        H, W = SIZES[name]
        out = gpu_case(a.views, H, W, a.reps)
        out["size"] = name
        if cpu is not None:
            out["cpu_numpy_rule"] = dict(cpu, extrapolated_s_per_scene=out["config"]["views"] * (a.views - 1) * H * W / cpu["tests_per_s"],
                                         note="EXTRAPOLATED from the small size by (pixel, view) tests, not measured at this size")
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
