#!/usr/bin/env python3
"""Time the image preparation's GPU steps (csrc/image_resample.hip) at the size the reference's pipelines
meet: one 1600 x 1200 RGB image -> 682 x 512 (``read_img`` in train mode for a 512 x 512 network input), whole and with the
512 x 512 centre window, and PIL's ``Image.resize(..., resample=Image.LANCZOS)`` on the same array on the host.  Device events
after a warm-up that is not timed, median of --reps; one JSON line:
  resize_ms              ops.resize_lanczos_u8(img, (682, 512)): the two passes, uint8 out
  resize_crop_f32_ms     the same with crop = the centre window and want_f32: what prepare_view launches per view
  prepare_view_ms        data.views.prepare_view in train mode (that plus K on the host)
  depth_nearest_crop_ms  ops.depth_nearest_crop of a 1200 x 1600 depth map to the same window
  upload_ms              the host -> device copy of the decoded image (pageable memory), the step the GPU path adds
  tables_cold_ms         host time of ops.lanczos_tables for the two axes on their first use (cached per pair of lengths after that)
  pil_ms                 PIL on the host, median of --reps; null where PIL is not installed
  equal_restatement      the GPU bytes equal tests/_lanczos_ref.py's on a 128-row band of the window (the whole image takes the
                         restatement half a second)
No speed bar is set: neither side had been measured when this script was written.
Usage:  python scripts/bench_image_prep.py [--reps 20] [--width 1600] [--height 1200] [--out-height 512] [--out-width 512]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import _lanczos_ref as LR  # noqa: E402
from wild_deep_mvs_amd import ops  # noqa: E402
from wild_deep_mvs_amd.data import views  # noqa: E402


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


def host_timed(fn, reps):
    fn()
    s = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        s.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(s))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--width", type=int, default=1600)
    ap.add_argument("--height", type=int, default=1200)
    ap.add_argument("--out-height", type=int, default=512)
    ap.add_argument("--out-width", type=int, default=512)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X: there is no CPU path to time"
    img = LR.random_image(a.height, a.width, 3, seed=0)
    img[:, :, 1] = (np.add.outer(np.arange(a.height), np.arange(a.width)) // 5 % 256).astype(np.uint8)
    r, (rw, rh), crop = views.view_geometry(a.width, a.height, "train", a.out_height, a.out_width)
    t0 = time.perf_counter()
    ops.lanczos_tables(a.width, rw)
    ops.lanczos_tables(a.height, rh)
    tables_ms = 1e3 * (time.perf_counter() - t0)
    host = torch.from_numpy(img)
    dev, upload_ms = timed(lambda: host.cuda(), a.reps)
    K = np.array([[1500.0, 0.0, a.width / 2], [0.0, 1500.0, a.height / 2], [0.0, 0.0, 1.0]], dtype=np.float32)
    depth = torch.rand((a.height, a.width), device="cuda") * 10
    _, whole_ms = timed(lambda: ops.resize_lanczos_u8(dev, (rw, rh)), a.reps)
    (got, _), crop_ms = timed(lambda: ops.resize_lanczos_u8(dev, (rw, rh), crop=crop, want_f32=True), a.reps)
    _, view_ms = timed(lambda: views.prepare_view(dev, K, "train", a.out_height, a.out_width), a.reps)
    x0, y0, cw, ch = crop
    _, depth_ms = timed(lambda: ops.depth_nearest_crop(depth, (rh, rw), crop=(y0, x0, ch, cw), min_d=1.0, max_d=9.0), a.reps)
    # a band of the window against the restatement: the horizontal pass whole, the vertical pass on the band's rows
    band = min(128, ch)
    tmp = LR.resample_pass(img, rw, 1) if rw != a.width else img
    coeff, bounds, _ = LR.tables(a.height, rh)
    want = np.empty((band, cw, 3), dtype=np.uint8)
    for k in range(band):
        first, n = bounds[y0 + k]
        acc = (1 << 21) + np.tensordot(coeff[y0 + k, :n], tmp[first:first + n, x0:x0 + cw].astype(np.int64), axes=(0, 0))
        want[k] = np.clip(acc >> 22, 0, 255)
    same = bool(np.array_equal(got[:band].cpu().numpy(), want)) if rh != a.height else None
    try:
        from PIL import Image
        pil = Image.fromarray(img)
        pil_ms = host_timed(lambda: pil.resize((rw, rh), resample=Image.LANCZOS), a.reps)
    except ImportError:
        pil_ms = None
    print(json.dumps({"case": f"{a.width} x {a.height} RGB -> {rw} x {rh}, window {cw} x {ch} at ({x0}, {y0})", "device": torch.cuda.get_device_name(0),
                      "reps": a.reps, "resize_ms": whole_ms, "resize_crop_f32_ms": crop_ms, "prepare_view_ms": view_ms,
                      "depth_nearest_crop_ms": depth_ms, "upload_ms": upload_ms, "tables_cold_ms": tables_ms, "pil_ms": pil_ms,
                      "equal_restatement": same}), flush=True)


if __name__ == "__main__":
    main()
