#!/usr/bin/env python3
"""Time the trainer's loss tail and the depth-map scoring with ``Trainer.loss_engine`` "torch" and "pscv" (csrc/depth_gt.hip;
INTEGRATION.md section 2l) at the training shape: b = 1, five views, 512 x 640, supervised.

  tail     ``Trainer.loss_tail`` on ready-made network outputs, then ``backward`` to the gradients of those outputs:
             mvsnet   1 term   (one depth map of 128 x 160)
             vis      15 terms (three scales of 64 x 80, 128 x 160 and 256 x 320, each with four pair maps and log-uncertainties)
  scoring  ``Trainer.scores``: a 128 x 160 estimate against the 512 x 640 ground truth (EPE, 1 px and 3 px error rates)

The tail is launch- and wait-bound, so the clock is the host's around ``--iters`` iterations that end in a device synchronise (the
time a training loop would see); the two engines alternate, region by region, in one process.  ``--regions`` regions (at least 5)
after a warm-up that is not timed; min / median / max of the per-iteration time in one JSON line, with the launch counts of the
engine path as the code states them and the largest difference between the two engines' losses and gradients.
Usage:  python scripts/bench_gt_loss.py [--regions 7] [--iters 50] [--height 512] [--width 640]"""
import argparse
import json
import os
import sys
import time
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from wild_deep_mvs_amd.models.trainer import Trainer  # noqa: E402

VIEWS = 5


def make_sample(H, W, gen):
    lo, hi = torch.full((1, VIEWS), 2.0), torch.full((1, VIEWS), 6.0)
    depth = 3.0 + 2.0 * torch.rand(1, 1, H, W, generator=gen)
    mask = (torch.rand(1, 1, H, W, generator=gen) > 0.3).float()
    imgs = torch.rand(1, VIEWS, 3, H, W, generator=gen)
    return {k: v.cuda() for k, v in dict(imgs=imgs, depth=depth, mask=mask, depth_min=lo, depth_max=hi).items()}


def make_outputs(arch, H, W, gen):
    """What the network hands to the loss tail, as leaves that take gradients."""
    leaf = lambda *shape: (3.0 + 2.0 * torch.rand(*shape, generator=gen)).cuda().requires_grad_()
    unc = lambda *shape: torch.randn(*shape, generator=gen).cuda().requires_grad_()
    if arch == "mvsnet":
        return dict(depth_est_list=[leaf(1, H // 4, W // 4)], depth_pair_list=[])
    sizes = [(H // 8, W // 8), (H // 4, W // 4), (H // 2, W // 2)]
    return dict(depth_est_list=[leaf(1, h, w) for h, w in sizes],
                depth_pair_list=[[(leaf(1, 1, h, w), (unc(1, 1, h, w),)) for _ in range(VIEWS - 1)] for h, w in sizes])


def leaves(outputs):
    out = list(outputs["depth_est_list"])
    for pairs in outputs["depth_pair_list"]:
        for d, (u,) in pairs:
            out += [d, u]
    return out


def regions(fns, n_regions, iters):
    """fns: {name: callable}; every region runs each callable ``iters`` times between two synchronises, the names alternating."""
    for fn in fns.values():                                        # warm-up: code objects, allocator, autograd
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in fns}
    for _ in range(n_regions):
        for name, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                fn()
            torch.cuda.synchronize()
            ms[name].append(1e3 * (time.perf_counter() - t0) / iters)
    return {name: dict(min=float(np.min(v)), median=float(np.median(v)), max=float(np.max(v))) for name, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=640)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gt_loss: needs an MI355X (a time taken elsewhere says nothing)")
    if a.regions < 5:
        raise SystemExit("bench_gt_loss: at least 5 regions")
    gen = torch.Generator().manual_seed(0)
    sample = make_sample(a.height, a.width, gen)
    src_idx = list(range(1, VIEWS))
    result = {"case": f"b=1, {VIEWS} views, {a.height}x{a.width}, supervised", "regions": a.regions, "iters": a.iters,
              "clock": "host, per iteration of a region that ends in a device synchronise"}
    for arch, label, terms in (("mvsnet", "mvsnet_tail", 1), ("vis_mvsnet", "vis_tail", 15)):
        outputs = make_outputs(arch, a.height, a.width, gen)
        trainers, fns, checks = {}, {}, {}
        for engine in ("torch", "pscv"):
            tr = Trainer(None, types.SimpleNamespace(architecture=arch, upsample_training=False, occ_masking=False, supervised=True,
                                                     num_im_train=VIEWS, print_every=1, dataset="dtu_yao", geom_clamping=0.01))
            tr.loss_engine = engine
            trainers[engine] = tr

            def tail(tr=tr):
                for x in leaves(outputs):
                    x.grad = None
                loss = tr.loss_tail(outputs, sample, sample, 0, src_idx)
                loss.backward()
                return loss
            fns[engine] = tail
            loss = tail()
            checks[engine] = (float(loss.detach()), torch.cat([x.grad.flatten().double() for x in leaves(outputs)]))
        (lt, gt), (lp, gp) = checks["torch"], checks["pscv"]
        result[label] = dict(terms=terms, ms=regions(fns, a.regions, a.iters), launches_pscv=dict(forward=2, backward=1),
                             loss_rel_diff=abs(lp - lt) / abs(lt), grad_max_rel_diff=float((gp - gt).abs().max() / gt.abs().max()))
    est = (3.0 + 2.0 * torch.rand(1, a.height // 4, a.width // 4, generator=gen)).cuda()
    gt, mask = sample["depth"][:, 0], sample["mask"][:, 0]
    step = ((sample["depth_max"] - sample["depth_min"]) / 128)[:, 0]
    fns, vals = {}, {}
    for engine in ("torch", "pscv"):
        tr = trainers[engine]
        fns[engine] = lambda tr=tr: tr.scores(est, gt, mask, step)
        vals[engine] = {k: float(v) for k, v in fns[engine]().items()}
    result["scoring"] = dict(ms=regions(fns, a.regions, a.iters), launches_pscv=2,
                             max_rel_diff=max(abs(vals["pscv"][k] - v) / abs(v) for k, v in vals["torch"].items()))
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
