#!/usr/bin/env python3
"""Time the scene set-up from a sparse model (csrc/scene_setup.hip) on a synthetic YFCC-sized scene:
2 000 images, 300 000 points, track lengths from a heavy-tailed distribution of mean about 8 (tests/_scene_setup_ref.py).
Device events after a warm-up that is not timed, median of 5 (per launch for the C-ABI calls); one JSON line:
  pair_counts_ms       pscv_sparse_pair_counts (the zero-fill and the pair kernel), events around the launch alone;
                       pair_counts_op_ms is ops.sparse_pair_counts = that launch plus the op's index validation, which reads
                       three or four flags back to the host; atomics = L^2 adds into adj plus the adds into adj_tri it reports, atomics_per_s against
                       the scattered rate of profiles/r01_ubench_global_atomic_rate.txt
  obs_depths_ms, sort_ms, percentiles_ms    the three steps of ops.sparse_depth_ranges, and depth_ranges_ms for the whole op
  select_ms            the torch selection of utils/colmap_utils.py:select_source_views
scripts/time_reference_cpu.py --scene-setup times the numpy restatement on the same scene.
Usage:  python scripts/bench_scene_setup.py [--reps 5] [--images 2000] [--points 300000] [--mean 8]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import _scene_setup_ref as SR  # noqa: E402
from wild_deep_mvs_amd import ops  # noqa: E402
from wild_deep_mvs_amd.utils.colmap_utils import select_source_views  # noqa: E402

SCATTERED_ATOMICS_PER_S = 21.2e9          # profiles/r01_ubench_global_atomic_rate.txt, "agent scattered"


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
    return out, float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--images", type=int, default=2000)
    ap.add_argument("--points", type=int, default=300000)
    ap.add_argument("--mean", type=float, default=8.0)
    a = ap.parse_args()
    sc = SR.bench_scene(a.images, a.points, a.mean)
    d = lambda x, dt: torch.as_tensor(np.ascontiguousarray(x), dtype=dt).cuda()
    xyz, off, img = d(sc["xyz"], torch.float64), d(sc["track_off"], torch.int64), d(sc["track_img"], torch.int32)
    oi, op, R, t = d(sc["obs_img"], torch.int32), d(sc["obs_pt"], torch.int32), d(sc["R"], torch.float32), d(sc["t"], torch.float32)
    lengths = np.diff(sc["track_off"])
    ops.sparse_pair_counts(xyz, off, img, R, t, 5.0)                    # warm-up outside the timer: code-object load, allocator
    ops.sparse_depth_ranges(xyz, oi, op, R, t)
    with ops.EventTimer() as tm:
        (adj, tri), pair_op_ms = timed(lambda: ops.sparse_pair_counts(xyz, off, img, R, t, 5.0), a.reps)
        _, whole_ms = timed(lambda: ops.sparse_depth_ranges(xyz, oi, op, R, t), a.reps)
    torch.cuda.synchronize()
    per_launch = {}
    for name, e0, e1 in tm.records:
        per_launch.setdefault(name, []).append(e0.elapsed_time(e1))
    parts = {k: float(np.median(v)) for k, v in per_launch.items()}       # median over the launches of each name
    pair_ms = parts["sparse_pair_counts"]
    atomics = int((lengths ** 2).sum()) + int(tri.sum())
    keys = torch.randint(0, 2 ** 62, (len(sc["obs_img"]),), device="cuda")
    _, sort_ms = timed(lambda: torch.sort(keys), a.reps)
    _, select_ms = timed(lambda: select_source_views(adj, tri, 4), a.reps)
    print(json.dumps({"case": f"{a.images} images x {a.points} points", "observations": int(lengths.sum()), "mean_track": float(lengths.mean()),
                      "longest_track": int(lengths.max()), "ordered_pairs": int((lengths ** 2).sum()), "atomics": atomics,
                      "pair_counts_ms": pair_ms, "pair_counts_op_ms": pair_op_ms, "atomics_per_s": atomics / (pair_ms * 1e-3),
                      "share_of_scattered_atomic_rate": atomics / (pair_ms * 1e-3) / SCATTERED_ATOMICS_PER_S,
                      "obs_depths_ms": parts["sparse_obs_depths"], "sort_ms": sort_ms, "percentiles_ms": parts["segment_percentiles"],
                      "depth_ranges_ms": whole_ms, "select_ms": select_ms}), flush=True)


if __name__ == "__main__":
    main()
