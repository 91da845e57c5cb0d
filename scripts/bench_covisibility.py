#!/usr/bin/env python3
"""Time ops.view_covisibility (csrc/view_covis.hip) on shuffled synthetic YFCC-like collections: V = 50, 200 and 1000 ragged views
around 128 x 160 at stride 4.  Device events around the call after a warm-up, median of 5; one JSON line per case with ms and
projections/s (a projection = one valid sample into one target view).  The V = 50 line also carries the time of the numpy rule
(tests/_covisibility_ref.py) on the same scene.  A last line times, on 64 of those views (PSCV_FUSE_MAX_VIEWS, the most a fusion
takes), the overlap pass next to one fusion pass (ops.colmap_fuse_pass of view 0) and the whole ops.colmap_fuse with the lists it
gave.
Usage:  python scripts/bench_covisibility.py [--reps 5] [--views 50,200,1000] [--stride 4]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from wild_deep_mvs_amd import ops, synthetic  # noqa: E402
from wild_deep_mvs_amd.utils.colmap_model import overlap_from_covisibility  # noqa: E402

H, W, E = 128, 160, 0.01


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
    ap.add_argument("--views", default="50,200,1000")
    ap.add_argument("--stride", type=int, default=4)
    a = ap.parse_args()
    for V in [int(v) for v in a.views.split(",")] + [0]:
        fusion = V == 0
        V = ops.L.FUSE_MAX_VIEWS if fusion else V
        sc = synthetic.make_permuted_yfcc_fusion_scene(V, H, W, seed=0, perm_seed=0, spacing=0.25 if V <= 64 else 2.0 / np.sqrt(V))
        cams = ops.geo_filter_cams(sc["K"], sc["R"], sc["t"])
        depths, cams_d = [d.cuda() for d in sc["depths"]], cams.cuda()
        counts, ms = timed(lambda: ops.view_covisibility(depths, cams_d, stride=a.stride, max_depth_error=E), a.reps)
        samples = sum(int((d[::a.stride, ::a.stride] > 0).sum()) for d in sc["depths"])
        med = float(np.median(ms))
        line = {"case": f"{V}x{H}x{W}" + ("+fusion" if fusion else ""), "views": V, "stride": a.stride, "samples": samples,
                "projections": samples * (V - 1), "ms_median": med, "ms_all": [round(x, 3) for x in ms],
                "projections_per_s": samples * (V - 1) / (med * 1e-3), "consistent_pairs": int((counts[..., 1] > 0).sum())}
        if V == 50 and not fusion:
            from tests import _covisibility_ref as VR
            t0 = time.perf_counter()
            want, border, _ = VR.covisibility([d.numpy() for d in sc["depths"]], cams.numpy(), stride=a.stride, max_depth_error=E)
            line["numpy_ms"] = (time.perf_counter() - t0) * 1e3
            line["max_abs_diff_vs_numpy"] = int(np.abs(counts.cpu().numpy() - want).max())
            line["borderline"] = int(border.sum())
        if fusion:
            colors = [c.cuda() for c in sc["colors"]]
            lists = overlap_from_covisibility(counts, 50)
            kw = dict(max_depth_error=E, max_reproj_error=1.0, min_num_pixels=3)
            fused = lambda: [torch.zeros(d.shape, dtype=torch.uint8, device="cuda") for d in depths]
            _, ms1 = timed(lambda: ops.colmap_fuse_pass(0, depths, colors, cams_d, lists, fused(), **kw), a.reps)
            out, msf = timed(lambda: ops.colmap_fuse(depths, colors, cams_d, lists, **kw), a.reps)
            line.update({"fuse_pass_ms_median": float(np.median(ms1)), "fuse_all_ms_median": float(np.median(msf)),
                         "points": int(out[0].shape[0]), "mean_list_length": float(np.mean([len(l) for l in lists]))})
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
