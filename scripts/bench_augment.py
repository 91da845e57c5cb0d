#!/usr/bin/env python3
"""Time the training-view augmentation (csrc/image_augment.hip) at the size of BlendedMVS's training
tuple: 5 views of 576 x 768 RGB, each with both colour steps and a 3 x 3 blur, whole images out.  Device events after a warm-up that
is not timed, median of --reps; one JSON line:
  augment_ms         ops.augment_views: the launch pair (pscv_augment_grey_sums, pscv_augment_apply) with its host side
  apply_only_ms      the same records without contrast: no sum launch
  upload_ms          the host -> device copy of the five decoded images (pageable memory)
  host_ms            the same augmentation on the host: PIL's ImageEnhance for the colour steps, then numpy for /255 and the blur
                     (tests/_augment_ref.py:blur32; the reference uses cv2.filter2D there, which is not a dependency of this
                     project), median of --host-reps; null where PIL is not installed
  equal_restatement  the GPU's bits equal tests/_augment_ref.py's on every view
No speed bar is set.
Usage:  python scripts/bench_augment.py [--reps 20] [--host-reps 3] [--views 5] [--height 576] [--width 768]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import _augment_ref as AR  # noqa: E402
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
    s = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        s.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(s))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--views", type=int, default=5)
    ap.add_argument("--height", type=int, default=576)
    ap.add_argument("--width", type=int, default=768)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X: there is no CPU path to time"
    imgs = np.stack([AR.random_image(a.height, a.width, seed=v) for v in range(a.views)])
    modes = views.BLUR_MODES
    recs = [views.ViewAugmentation(order=("brightness", "contrast") if v % 2 else ("contrast", "brightness"), brightness=0.85 + 0.07 * v,
                                   contrast=0.4 + 0.25 * v, blur_mode=modes[v % 4], ksize=3) for v in range(a.views)]
    no_contrast = [views.ViewAugmentation(order=r.order, brightness=r.brightness, blur_mode=r.blur_mode, ksize=3) for r in recs]
    host = torch.from_numpy(imgs)
    dev, upload_ms = timed(lambda: host.cuda(), a.reps)
    got, augment_ms = timed(lambda: ops.augment_views(dev, recs), a.reps)
    _, apply_ms = timed(lambda: ops.augment_views(dev, no_contrast), a.reps)
    got = got.cpu().numpy()
    same = all(np.array_equal(got[v].view(np.int32), AR.augment(imgs[v], recs[v].steps(), recs[v].blur_kernel()).view(np.int32))
               for v in range(a.views))
    try:
        from PIL import Image, ImageEnhance

        def on_host():
            for v, r in enumerate(recs):
                pil = Image.fromarray(imgs[v])
                for name, f in r.steps():
                    pil = (ImageEnhance.Brightness if name == "brightness" else ImageEnhance.Contrast)(pil).enhance(f)
                AR.blur32(np.array(pil, dtype=np.float32) / 255., r.blur_kernel())

        host_ms = host_timed(on_host, a.host_reps)
    except ImportError:
        host_ms = None
    print(json.dumps({"case": f"{a.views} x {a.width} x {a.height} RGB, both colour steps and a 3 x 3 blur per view", "device": torch.cuda.get_device_name(0),
                      "reps": a.reps, "augment_ms": augment_ms, "apply_only_ms": apply_ms, "upload_ms": upload_ms, "host_ms": host_ms,
                      "host_reps": a.host_reps, "equal_restatement": bool(same)}), flush=True)


if __name__ == "__main__":
    main()
