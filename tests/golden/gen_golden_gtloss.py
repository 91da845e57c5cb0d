#!/usr/bin/env python3
"""Generate tests/golden/gtloss_tiny.npz, the fixture of the loss reductions and depth-map scores.

Inputs (b = 2): a ground truth of 24 x 48 with a random mask (about 30 % invalid) and per-image depth intervals that differ;
depth maps at 24x48, 12x24, 6x12, 8x16 and 12x48 (ratios 1, 2, 4, 3 and the mixed (2, 1)), each with two pair maps and their
log-uncertainties; an SSIM-like loss map with a float and a bool mask; estimates of 6x12, 24x48 and 7x13 for the scores.

Expected values come from the reference's OWN ``bayesian_version_loss`` and its five metric functions (models/utils.py, loaded from
the reference tree with ``torchvision`` stood for by an empty module, here only) and from torch's ``F.interpolate`` -- in fp64
where it feeds an expected scalar, in fp32 for the resized ground truth itself.  Arrays only.

The seed of the score inputs is the first for which no valid pixel lies within 1e-3 (relative) of a threshold, so that the counts
of the fp32 kernel and of the fp64 expectation cannot differ by rounding.  The file is written with fixed zip timestamps: running
the script again gives the same bytes.  Usage:  python tests/golden/gen_golden_gtloss.py"""
from __future__ import annotations

import importlib.util
import io
import os
import sys
import types
import zipfile

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)
from gen_golden import REF  # noqa: E402  (where the reference tree lies)
from tests import _gt_loss_ref as R  # noqa: E402

B, H, W = 2, 24, 48
SCALES = {"s1": (24, 48), "s2": (12, 24), "s4": (6, 12), "s3": (8, 16), "s21": (12, 48)}
SCORE_SIZES = {"m4": (6, 12), "m1": (24, 48), "mf": (7, 13)}
THRESHOLDS, REL_THRESHOLDS = (1.0, 3.0), (1.05, 1.25)
MARGIN = 1e-3
BLOCK_PIXELS = 1024                                  # pixels per workgroup and step of the reduce launch (csrc/loss_plan.h)


def reference_utils():
    sys.dont_write_bytecode = True
    for name in ("torchvision", "torchvision.utils"):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    sys.modules["torchvision"].utils = sys.modules["torchvision.utils"]
    spec = importlib.util.spec_from_file_location("_reference_models_utils", os.path.join(REF, "models", "utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def t64(x):
    return torch.from_numpy(np.asarray(x, dtype=np.float64))


def loss_inputs():
    rng = np.random.default_rng(2024)
    a = {}
    yy, xx = np.mgrid[0:H, 0:W]
    base = 3.5 + 0.4 * np.sin(xx / 9.0) + 0.3 * np.cos(yy / 5.0)
    a["gt"] = (base[None] + rng.normal(0, 0.05, (B, H, W))).astype(np.float32)
    a["gt_mask"] = (rng.random((B, H, W)) >= 0.3).astype(np.float32)
    a["interval"] = np.array([0.031, 0.047], dtype=np.float32)
    for name, (h, w) in SCALES.items():
        gd, _ = R.gt_down(a["gt"], np.ones((B, H, W), np.float32), h, w)
        a[f"{name}_d"] = (gd + rng.normal(0, 0.08, (B, h, w))).astype(np.float32)
        a[f"{name}_d"][:, 1, 2] = gd[:, 1, 2]        # d == gt_down: sign(0) = 0
        for j in range(2):
            a[f"{name}_p{j}_d"] = (gd + rng.normal(0, 0.12, (B, 1, h, w))[:, 0]).astype(np.float32)
            a[f"{name}_p{j}_u"] = rng.normal(0.3, 0.8, (B, 1, h, w)).astype(np.float32)
    a["l"] = rng.random((B, 3, H, W)).astype(np.float32) * 0.9
    a["l_u"] = rng.normal(0.0, 0.7, (B, 3, H, W)).astype(np.float32)
    a["l_mask_f"] = (rng.random((B, 3, H, W)) >= 0.4).astype(np.float32)
    a["l_mask_b"] = rng.random((B, 3, H, W)) >= 0.25
    return a


def loss_expectations(a, ref):
    out = {}
    gt, gm = t64(a["gt"]).unsqueeze(1), t64(a["gt_mask"]).unsqueeze(1)
    interval = t64(a["interval"]).view(B, 1, 1, 1)
    for name, (h, w) in SCALES.items():
        g64 = F.interpolate(gt, size=(h, w), mode="bilinear", align_corners=False)
        m64 = (F.interpolate(gm, size=(h, w), mode="bilinear", align_corners=False) == 1).double()
        g32 = F.interpolate(torch.from_numpy(a["gt"]).unsqueeze(1), size=(h, w), mode="bilinear", align_corners=False)
        m32 = F.interpolate(torch.from_numpy(a["gt_mask"]).unsqueeze(1), size=(h, w), mode="bilinear", align_corners=False) == 1
        assert torch.equal(m32, m64.bool())
        out[f"{name}_gt_down"], out[f"{name}_mask_down"] = g32[:, 0].numpy(), m32[:, 0].numpy()
        inv = R.invalid_taps(a["gt_mask"], h, w)
        ntaps = (1 if (H // h) % 2 else 2) * (1 if (W // w) % 2 else 2)
        for k in range(1, min(ntaps, 3) + 1):
            assert (inv == k).any(), f"{name}: no pixel with exactly {k} invalid taps"
        assert (inv == 0).any()
        d = t64(a[f"{name}_d"]).unsqueeze(1)
        l = torch.abs(d - g64) / interval
        out[f"{name}_plain"] = np.float64(torch.sum(l * m64) / torch.sum(m64))      # trainer.py:157 (the supervised masked mean)
        out[f"{name}_count"] = np.float64(m64.sum())
        for j in range(2):
            dp = t64(a[f"{name}_p{j}_d"]).unsqueeze(1)
            lp = torch.abs(dp - g64) / interval
            out[f"{name}_p{j}_bayes"] = np.float64(ref.bayesian_version_loss(lp, t64(a[f"{name}_p{j}_u"]), m64))
    l, u = t64(a["l"]), t64(a["l_u"])
    mf, mb = t64(a["l_mask_f"]), t64(a["l_mask_b"].astype(np.float64))
    out["l_plain_f"] = np.float64(torch.sum(l * mf) / torch.sum(mf))               # trainer.py:159-163 (mask not empty)
    out["l_plain_b"] = np.float64(torch.sum(l * mb) / torch.sum(mb))
    out["l_bayes_f"] = np.float64(ref.bayesian_version_loss(l, u, mf))
    out["l_bayes_b"] = np.float64(ref.bayesian_version_loss(l, u, mb))
    out["l_bayes_empty"] = np.float64(ref.bayesian_version_loss(l, u, torch.zeros_like(mf)))
    return out


def score_inputs(seed):
    rng = np.random.default_rng(1000 + seed)
    a = {}
    yy, xx = np.mgrid[0:H, 0:W]
    a["m_gt"] = np.stack([3.0 + 0.004 * xx + 0.006 * yy, 4.5 - 0.005 * xx + 0.003 * yy]).astype(np.float32)
    a["m_gt"] *= (1.0 + rng.uniform(-0.002, 0.002, (B, H, W))).astype(np.float32)
    a["m_mask"] = (rng.random((B, H, W)) >= 0.3).astype(np.float32)
    a["m_min"] = np.array([[2.0, 2.1, 1.9], [2.5, 2.4, 2.6]], dtype=np.float32)
    a["m_max"] = np.array([[6.0, 6.2, 5.8], [7.5, 7.7, 7.2]], dtype=np.float32)
    for name, (h, w) in SCORE_SIZES.items():
        ys, xs = (np.arange(h) + 0.5) * H / h - 0.5, (np.arange(w) + 0.5) * W / w - 0.5
        yg, xg = np.meshgrid(ys, xs, indexing="ij")
        plane = np.stack([3.0 + 0.004 * xg + 0.006 * yg, 4.5 - 0.005 * xg + 0.003 * yg])
        err = rng.uniform(-0.004, 0.004, (B, h, w))
        outlier = rng.random((B, h, w)) < 0.02
        err = np.where(outlier, rng.choice([-1.0, 1.0], (B, h, w)) * rng.uniform(0.1, 0.5, (B, h, w)), err)
        a[f"{name}_est"] = (plane * (1.0 + err)).astype(np.float32)
    return a


def score_expectations(a, ref):
    out = {}
    step = (a["m_max"][:, 0] - a["m_min"][:, 0]) / np.float32(128)
    st = t64(step).view(B, 1, 1)
    gt, valid = t64(a["m_gt"]) / st, torch.from_numpy(a["m_mask"]) > 0.5
    for name in SCORE_SIZES:
        est = F.interpolate(t64(a[f"{name}_est"]).unsqueeze(1), (H, W), mode="bilinear", align_corners=False).squeeze(1) / st
        out[f"{name}_EPE"] = np.float64(ref.AbsDepthError_metrics(est, gt, valid))
        out[f"{name}_Rel"] = np.float64(ref.RelDepthError_metrics(est, gt, valid))
        out[f"{name}_SqRel"] = np.float64(ref.SquareRelDepthError_metrics(est, gt, valid))
        out[f"{name}_thres"] = np.array([float(ref.Thres_metrics(est, gt, valid, t)) for t in THRESHOLDS])
        out[f"{name}_rel_thres"] = np.array([float(ref.Rel_Thres_metrics(est, gt, valid, r)) for r in REL_THRESHOLDS])
        ad = (est - gt).abs()
        ratio = torch.max(est / gt, gt / est)
        out[f"{name}_count"] = valid.sum(dim=(1, 2)).numpy().astype(np.float64)
        out[f"{name}_thres_counts"] = np.stack([((ad > t) & valid).sum(dim=(1, 2)).numpy() for t in THRESHOLDS], axis=1).astype(np.float64)
        out[f"{name}_rel_counts"] = np.stack([((ratio > r) & valid).sum(dim=(1, 2)).numpy() for r in REL_THRESHOLDS], axis=1).astype(np.float64)
    return out


def margin(a):
    step = (a["m_max"][:, 0] - a["m_min"][:, 0]) / np.float32(128)
    return min(R.threshold_margin(a[f"{n}_est"], a["m_gt"], a["m_mask"], step, THRESHOLDS, REL_THRESHOLDS) for n in SCORE_SIZES)


def write_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps: the same arrays give the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


def main():
    ref = reference_utils()
    arrays = loss_inputs()
    arrays.update(loss_expectations(arrays, ref))
    npix = B * H * W
    assert npix > BLOCK_PIXELS and npix % BLOCK_PIXELS, "a term must span more than one block and end in a ragged one"
    tried = []
    for seed in range(200):
        sc = score_inputs(seed)
        tried.append(margin(sc) > MARGIN)
        if tried[-1]:
            break
    else:
        raise SystemExit("no seed keeps every valid pixel 1e-3 away from the thresholds")
    print(f"score seed {seed} (of seeds 0..{seed}, {sum(tried)} qualified); margin {margin(sc):.3e}")
    arrays.update(sc)
    arrays.update(score_expectations(sc, ref))
    arrays.update(m_seed=np.int64(seed), m_thresholds=np.array(THRESHOLDS), m_rel_thresholds=np.array(REL_THRESHOLDS))
    # the restatement against what was just computed (a difference stops the script)
    for name, (h, w) in SCALES.items():
        g, m = R.gt_down(arrays["gt"], arrays["gt_mask"], h, w)
        assert np.array_equal(m, arrays[f"{name}_mask_down"]), name
        assert np.abs(g - arrays[f"{name}_gt_down"]).max() <= 2e-7 * np.abs(g).max(), name
    for name in SCORE_SIZES:
        step = (sc["m_max"][:, 0] - sc["m_min"][:, 0]) / np.float32(128)
        got = R.metrics(sc[f"{name}_est"], sc["m_gt"], sc["m_mask"], step, THRESHOLDS, REL_THRESHOLDS)
        assert np.array_equal(got["sums"][:, 2:4], arrays[f"{name}_thres_counts"]) and np.array_equal(got["sums"][:, 8:10], arrays[f"{name}_rel_counts"]), name
        assert abs(got["EPE"] - arrays[f"{name}_EPE"]) <= 1e-5 * arrays[f"{name}_EPE"], name
    path = os.path.join(HERE, "gtloss_tiny.npz")
    write_npz(path, arrays)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB, {len(arrays)} arrays)")


if __name__ == "__main__":
    main()
