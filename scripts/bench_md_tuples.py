#!/usr/bin/env python3
"""Time the MegaDepth tuple mining's GPU steps (csrc/scene_setup.hip) on a synthetic scene of MegaDepth
proportions: 2 000 images, 300 000 points, track lengths from a heavy-tailed distribution of mean about 8
(tests/_md_tuples_ref.py:bench_scene), T candidate tuples of V = 5 neighbouring images.  Device events after a warm-up that is
not timed, median of 5; one JSON line:
  pair_counts_op_ms        ops.sparse_pair_counts, the two matrices the candidates are picked from
  visible_depths_ms        pscv_tuple_visible_depths for all T tuples, events around the call (its two passes and the read-back of
                           the tuples); visible_depths_op_ms is ops.tuple_visible_depths = that plus the op's index validation
  restatement_s            the numpy restatement (tests/_md_tuples_ref.py:visible_depths) on the first --ref-tuples tuples, and
                           restatement_s_per_tuple; the reference's own triple loop (points x views x track, in Python) is not timed
No speed bar is set: neither side had been measured when this script was written.
Usage:  python scripts/bench_md_tuples.py [--reps 5] [--images 2000] [--points 300000] [--mean 8] [--tuples 512] [--views 5] [--ref-tuples 8]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import _md_tuples_ref as MR  # noqa: E402
from wild_deep_mvs_amd import ops  # noqa: E402


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
    ap.add_argument("--tuples", type=int, default=512)
    ap.add_argument("--views", type=int, default=5)
    ap.add_argument("--ref-tuples", type=int, default=8)
    a = ap.parse_args()
    sc = MR.bench_scene(a.images, a.points, a.mean)
    rng = np.random.default_rng(1)
    starts = rng.integers(0, a.images, a.tuples)
    tuples, K, sizes = MR.tuples_of(sc, np.stack([rng.permutation((s + np.arange(2 * a.views)) % a.images)[:a.views] for s in starts]))
    d = lambda x, dt: torch.as_tensor(np.ascontiguousarray(x), dtype=dt).cuda()
    xyz, off, img = d(sc["xyz"], torch.float64), d(sc["track_off"], torch.int64), d(sc["track_img"], torch.int32)
    R, t = d(sc["R"], torch.float32), d(sc["t"], torch.float32)
    tup, Kd, sd = d(tuples, torch.int32), d(K, torch.float32), d(sizes, torch.float64)
    _, pair_ms = timed(lambda: ops.sparse_pair_counts(xyz, off, img, R, t, 5.0), a.reps)
    with ops.EventTimer() as tm:
        out, op_ms = timed(lambda: ops.tuple_visible_depths(xyz, off, img, tup, Kd, R, t, sd), a.reps)
    torch.cuda.synchronize()
    call_ms = float(np.median([e0.elapsed_time(e1) for name, e0, e1 in tm.records if name == "tuple_visible_depths"]))
    n_pts = out[4].cpu().numpy()
    n_ref = min(a.ref_tuples, a.tuples)
    t0 = time.perf_counter()
    want = MR.visible_depths_batch(sc["xyz"], sc["track_off"], sc["track_img"], tuples[:n_ref], K[:n_ref], sc["R"], sc["t"], sizes[:n_ref])
    ref_s = time.perf_counter() - t0
    same = bool(np.array_equal(out[2].cpu().numpy()[:n_ref], want["min_row"]) and np.array_equal(out[3].cpu().numpy()[:n_ref], want["max_row"])
                and np.array_equal(n_pts[:n_ref], want["n_pts"]))
    lengths = np.diff(sc["track_off"])
    print(json.dumps({"case": f"{a.images} images x {a.points} points, {a.tuples} tuples of {a.views}", "observations": int(lengths.sum()),
                      "longest_track": int(lengths.max()), "mean_points_per_tuple": float(n_pts.mean()), "pair_counts_op_ms": pair_ms,
                      "visible_depths_ms": call_ms, "visible_depths_op_ms": op_ms, "visible_depths_us_per_tuple": 1e3 * call_ms / a.tuples,
                      "restatement_tuples": n_ref, "restatement_s": ref_s, "restatement_s_per_tuple": ref_s / n_ref,
                      "rows_equal_restatement": same}), flush=True)


if __name__ == "__main__":
    main()
