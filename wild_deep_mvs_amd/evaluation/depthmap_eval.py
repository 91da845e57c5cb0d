"""The depth-map protocol of the reference's ``depthmap_eval.py`` (lines 104-143, the numbers of the paper's depth-map tables) on
the engine: the estimate is upsampled bilinearly to the ground truth's size, both are divided by the depth step of view 0,
``(depth_max - depth_min) / 128``, and EPE and the 1 px / 3 px error rates are taken over the valid pixels of each image -- one
``ops.depth_metrics`` call per sample, no host wait.  ``Scores`` sums the results on the device over a loader and waits once.
The script's command line, loaders and plots are not mirrored."""
from __future__ import annotations

import torch

from .. import ops

NAMES = ("EPE", "1pxError", "3pxError")


def score(depth, gt, mask, depth_min, depth_max):
    """depth [b,h,w] (any size), gt / mask [b,H,W], depth_min / depth_max [b,n_views] (or [b]) -> {"EPE", "1pxError", "3pxError"}
    as 0-dim device tensors: the batch means of the per-image values (depthmap_eval.py:132-143)."""
    lo = depth_min[:, 0] if depth_min.dim() > 1 else depth_min
    hi = depth_max[:, 0] if depth_max.dim() > 1 else depth_max
    step = ((hi - lo) / 128).to(torch.float32)
    m = ops.depth_metrics(depth, gt, mask, step, thresholds=(1, 3))
    return {"EPE": m["EPE"], "1pxError": m["thres"][0], "3pxError": m["thres"][1]}


class Scores:
    """Running sums of ``score`` results, kept on the device: ``add`` never waits, ``result(n)`` is the one read."""

    def __init__(self):
        self.total = None
        self.count = 0

    def add(self, scores):
        row = torch.stack([scores[k] for k in NAMES])
        self.total = row if self.total is None else self.total + row
        self.count += 1

    def result(self, n=None):
        """Means over ``n`` samples (default: the number of ``add`` calls) as Python floats."""
        if self.total is None:
            raise ValueError("Scores.result: nothing was added")
        values = (self.total / float(self.count if n is None else n)).tolist()
        return dict(zip(NAMES, values))
