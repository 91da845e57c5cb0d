"""Synthetic plane-sweep inputs and deterministic network weights.

There are no datasets or checkpoints in the build environment, so the tests,
``bench.py``, ``__graft_entry__.smoke()`` and the golden-vector generator
(``tests/golden/gen_golden.py``) all draw their cameras, images, feature maps
and weights from here.  Everything is seeded through ``numpy.random.Generator``
(PCG64, platform independent) so that the same tensors can be re-created on the
GPU box without committing them.

The sample dict mirrors what the reference's dataset loaders hand to
``forward()`` (reference ``data/dtu_yao.py:133-146``): ``imgs`` [B,V,3,H,W],
``K``/``R`` [B,V,3,3], ``t`` [B,V,3,1], ``depth_min``/``depth_max`` [B,V].

Weights are *sharpened*: with PyTorch default initialisation the reference's
logits have a std of ~1e-6 over the depth axis, the softmax is uniform and the
depth map is independent of the warp, which would make
every depth-parity check vacuous.
"""
from __future__ import annotations

import math
from collections import OrderedDict
from typing import Dict, Mapping, Sequence, Tuple

import numpy as np
import torch


# --------------------------------------------------------------------------
# cameras / scenes
# --------------------------------------------------------------------------
def make_cameras(B: int, V: int, H: int, W: int, *, depth_min: float = None,
                 depth_max: float = None, behind_view: int = -1, rig: str = "probe",
                 dtype=torch.float32) -> Dict[str, torch.Tensor]:
    """Two pinhole rigs.

    ``rig="probe"`` (default; depth 2..6): reference camera at identity, source ``v`` rotated about the
    y axis by ``0.05 v (-1)^v`` rad and shifted ``0.1 v (-1)^v`` along x.

    ``rig="dtu"`` (depth 425..905 = 425 + 192 x 2.5, reference ``data/dtu_yao.py:109``): the geometry of
    Yao's DTU training set -- focal length 2.26 W (1446 px at 640), cameras on an arc around an object
    point 660 mm in front of the reference camera, looking at it: source ``v`` is rotated about the
    vertical axis through that point by ``5 ceil(v/2) (-1)^v`` degrees (baselines 58 / 115 mm) and tilted
    by ``1.5 v (-1)^(v//2)`` degrees about the horizontal axis, so epipolar lines are not image rows and
    one plane step moves a sample by 0.13-0.27 feature texels (0.03-0.1 in the probe rig).

    ``behind_view >= 0`` turns that source camera around (rotation by ~pi about
    y) so that every reference ray lands behind it -- the ``q_z <= 0`` branch of
    the warp (reference ``models/MVSNet/module.py:147-150``).
    """
    if rig not in ("probe", "dtu"):
        raise ValueError(f"unknown rig {rig!r}")
    if depth_min is None:
        depth_min = 2.0 if rig == "probe" else 425.0
    if depth_max is None:
        depth_max = 6.0 if rig == "probe" else 905.0
    K = torch.zeros(B, V, 3, 3, dtype=dtype)
    R = torch.zeros(B, V, 3, 3, dtype=dtype)
    t = torch.zeros(B, V, 3, 1, dtype=dtype)
    for b in range(B):
        for v in range(V):
            sgn = -1.0 if v % 2 else 1.0
            if rig == "probe":
                f = 0.9 * W * (1.0 + 0.02 * v + 0.01 * b)
                K[b, v] = torch.tensor([[f, 0.0, W / 2.0 + 0.5 * v],
                                        [0.0, f, H / 2.0 - 0.25 * v],
                                        [0.0, 0.0, 1.0]], dtype=dtype)
                a = 0.05 * v * sgn + 0.01 * b
                if v == behind_view:
                    a = math.pi - 0.1
                ca, sa = math.cos(a), math.sin(a)
                R[b, v] = torch.tensor([[ca, 0.0, sa], [0.0, 1.0, 0.0], [-sa, 0.0, ca]], dtype=dtype)
                t[b, v] = torch.tensor([[0.1 * v * sgn], [0.02 * v], [0.0]], dtype=dtype)
            else:
                f = 2.2595 * W * (1.0 + 0.002 * v)
                K[b, v] = torch.tensor([[f, 0.0, W / 2.0 + 11.6 * W / 640.0 + 0.5 * v],
                                        [0.0, f, H / 2.0 + 9.5 * H / 512.0 - 0.25 * v],
                                        [0.0, 0.0, 1.0]], dtype=dtype)
                zc = 660.0 + 5.0 * b
                th = math.radians(5.0 * ((v + 1) // 2)) * sgn + 0.002 * b
                ph = math.radians(1.5 * v) * (-1.0 if (v // 2) % 2 else 1.0)
                if v == behind_view:
                    th = math.pi - 0.1
                ct, st_, cp, sp = math.cos(th), math.sin(th), math.cos(ph), math.sin(ph)
                Ry = torch.tensor([[ct, 0.0, st_], [0.0, 1.0, 0.0], [-st_, 0.0, ct]], dtype=torch.float64)
                Rx = torch.tensor([[1.0, 0.0, 0.0], [0.0, cp, -sp], [0.0, sp, cp]], dtype=torch.float64)
                Rv = Rx @ Ry
                pivot = torch.tensor([[0.0], [0.0], [zc]], dtype=torch.float64)
                R[b, v] = Rv.to(dtype)
                t[b, v] = (pivot - Rv @ pivot).to(dtype)          # x_cam = Rv (x - pivot) + pivot: every camera sees the pivot at (0, 0, zc)
    dmin = torch.full((B, V), float(depth_min), dtype=dtype)
    dmax = torch.full((B, V), float(depth_max), dtype=dtype)
    return {"K": K, "R": R, "t": t, "depth_min": dmin, "depth_max": dmax}


def make_filter_scene(V: int, H: int, W: int, *, seed: int = 0, behind_view: int = -1, half_res_view: int = -1,
                      near_view: int = -1, baseline: float = 4.0) -> Dict[str, object]:
    """Depth maps of one tilted world plane seen by the ``make_cameras`` rig, for the geometric-consistency filter
    (the step after the hot path): ``depth`` [H,W] of view 0, ``src_depth`` list of V-1 maps, ``K``, ``R`` [V,3,3],
    ``t`` [V,3,1].  The plane depth is analytic per view (``d = (c + n.R^T t) / (n.R^T K^-1 p)``), so the maps are
    mutually consistent; smooth multiplicative perturbations of 0-3 % (independent per view) then move pixels to
    either side of the filter's 1 % / 1 px thresholds, and a block of gross outliers is planted in source 1.
    ``half_res_view`` renders that source at half resolution (own intrinsics): the filter takes per-source shapes.
    ``baseline`` scales the camera translations (wider baseline = larger triangulation angles); ``near_view`` keeps
    that source almost at the reference's position (triangulation angle below the 1 degree default)."""
    cam = make_cameras(1, V, H, W, behind_view=behind_view)
    K, R, t = cam["K"][0].clone(), cam["R"][0].clone(), cam["t"][0].clone() * baseline
    if near_view >= 0:
        t[near_view] = t[near_view] * 0.02
        R[near_view] = torch.eye(3)
    rng = np.random.default_rng(seed)
    n = torch.tensor([0.10, -0.06, 1.0])
    n = n / n.norm()
    c = 4.0 * float(n[2])
    maps = []
    for v in range(V):
        h, w = H, W
        Kv = K[v].clone()
        if v == half_res_view:
            h, w = H // 2, W // 2
            Kv[:2] *= 0.5
            K[v] = Kv
        ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
        p = torch.stack((xs, ys, torch.ones_like(xs)), dim=-1).reshape(-1, 3)
        ray = (p @ torch.inverse(Kv).t()) @ R[v]                       # R^T K^-1 p, as rows
        num = c + float(n @ (R[v].t() @ t[v]).squeeze(-1))
        d = (num / (ray @ n)).reshape(h, w)
        coarse = torch.from_numpy(rng.standard_normal((1, 1, max(h // 12, 2), max(w // 12, 2))).astype(np.float32))
        bump = torch.nn.functional.interpolate(coarse, size=(h, w), mode="bilinear", align_corners=False)[0, 0]
        d = d * (1.0 + 0.012 * bump * (0.3 if v == 0 else 1.0))
        if v == 1:
            d[h // 4:h // 2, w // 3:w // 2] *= 1.4                    # gross outliers
        maps.append(d.contiguous())
    return {"depth": maps[0], "src_depth": maps[1:], "K": K, "R": R, "t": t}


def make_fusion_scene(V: int, H: int, W: int, *, seed: int = 0, perturb: float = 0.004, outliers: bool = True,
                      half_res_view: int = -1, behind_view: int = -1, spacing: float = 0.25, exact: bool = False) -> Dict[str, object]:
    """Inputs of the depth-map fusion (the step after the geometric filter): V cameras on a square grid of ``spacing`` in the
    plane z = 0, each looking along +z with a small tilt towards the grid's centre, all seeing one tilted world plane
    ``n . X = c0`` at depth ~4 (focal 0.9 W).  Returns ``depths`` (V fp32 maps), ``colors`` (V uint8 [h,w,3]: a texture of the
    world position, so the views agree on colour up to small noise), ``K``, ``R`` [V,3,3], ``t`` [V,3,1] and the plane ``n``,
    ``c0``.  Depths are the analytic ray-plane distances; unless ``exact``, each view then gets a smooth multiplicative
    perturbation of up to ~``perturb`` (independent per view), view 1 a block of gross outliers (x 1.3) and every view a few
    masked (0) pixels.  ``half_res_view`` renders that view at half resolution (own intrinsics); ``behind_view`` turns that
    camera round to face a second plane behind the rig, so its points land behind every other camera and the others' behind
    it."""
    rng = np.random.default_rng(seed)
    n = np.array([0.10, -0.06, 1.0])
    n = n / np.linalg.norm(n)
    c0 = 4.0 * n[2]
    g = int(math.ceil(math.sqrt(V)))
    K, R, t, depths, colors = [], [], [], [], []
    for v in range(V):
        h, w = (H // 2, W // 2) if v == half_res_view else (H, W)
        f = 0.9 * w
        Kv = np.array([[f, 0.0, w / 2.0 + 0.3 * (v % 3)], [0.0, f, h / 2.0 - 0.2 * (v % 2)], [0.0, 0.0, 1.0]])
        gx, gy = v % g - (g - 1) / 2.0, v // g - (g - 1) / 2.0
        c = np.array([gx * spacing, gy * spacing, 0.0])
        ay, ax = -0.25 * gx * spacing / 4.0, 0.25 * gy * spacing / 4.0       # tilt a quarter of the way towards the centre line
        if v == behind_view:
            ay = math.pi - 0.05
        cy, sy, cx, sx = math.cos(ay), math.sin(ay), math.cos(ax), math.sin(ax)
        Ry = np.array([[cy, 0.0, sy], [0.0, 1.0, 0.0], [-sy, 0.0, cy]])
        Rx = np.array([[1.0, 0.0, 0.0], [0.0, cx, -sx], [0.0, sx, cx]])
        Rv = Rx @ Ry
        tv = -Rv @ c
        nv, cv = (n, c0) if v != behind_view else (np.array([0.0, 0.05, 1.0]) / np.linalg.norm([0.0, 0.05, 1.0]), -4.0)
        ys, xs = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
        p = np.stack((xs, ys, np.ones_like(xs)), axis=-1).reshape(-1, 3)
        ray = p @ np.linalg.inv(Kv).T @ Rv                                    # R^T K^-1 p, as rows
        d = ((cv - nv @ c) / (ray @ nv)).reshape(h, w)
        X = c + d.reshape(-1, 1) * ray
        col = np.stack((128 + 100 * np.sin(3.1 * X[:, 0]), 128 + 100 * np.sin(2.3 * X[:, 1] + 1.0),
                        128 + 100 * np.cos(1.7 * (X[:, 0] + X[:, 1]))), axis=-1).reshape(h, w, 3)
        if not exact:
            col = col + rng.normal(0.0, 2.0, col.shape)
            coarse = torch.from_numpy(rng.standard_normal((1, 1, max(h // 10, 2), max(w // 10, 2))))
            bump = torch.nn.functional.interpolate(coarse, size=(h, w), mode="bilinear", align_corners=False)[0, 0].numpy()
            d = d * (1.0 + perturb * np.tanh(bump))
            if v == 1 and outliers:
                d[h // 4:h // 2, w // 3:w // 2] *= 1.3
            d[rng.random((h, w)) < 0.01] = 0.0
        K.append(Kv); R.append(Rv); t.append(tv.reshape(3, 1))
        depths.append(torch.from_numpy(d.astype(np.float32)).contiguous())
        colors.append(torch.from_numpy(np.clip(np.rint(col), 0, 255).astype(np.uint8)).contiguous())
    f32 = lambda a: torch.from_numpy(np.stack(a).astype(np.float32))
    return {"depths": depths, "colors": colors, "K": f32(K), "R": f32(R), "t": f32(t), "n": n, "c0": c0}


def make_scene(B: int, V: int, H: int, W: int, *, seed: int = 0, depth_min: float = None,
               depth_max: float = None, behind_view: int = -1, rig: str = "probe") -> Dict[str, torch.Tensor]:
    """Full sample dict with smooth-ish random images in [0, 1)."""
    rng = np.random.default_rng(seed)
    # low-frequency content + noise so that the 2D feature nets see structure
    coarse = rng.random((B, V, 3, max(H // 8, 1), max(W // 8, 1)), dtype=np.float32)
    coarse_t = torch.from_numpy(coarse).reshape(B * V, 3, coarse.shape[-2], coarse.shape[-1])
    smooth = torch.nn.functional.interpolate(coarse_t, size=(H, W), mode="bilinear", align_corners=False)
    noise = torch.from_numpy(rng.random((B * V, 3, H, W), dtype=np.float32))
    imgs = (0.7 * smooth + 0.3 * noise).reshape(B, V, 3, H, W).contiguous()
    out = make_cameras(B, V, H, W, depth_min=depth_min, depth_max=depth_max, behind_view=behind_view, rig=rig)
    out["imgs"] = imgs
    return out


def make_photo_case(B: int, V: int, H: int, W: int, *, seed: int = 0, behind_view: int = -1) -> Dict[str, torch.Tensor]:
    """Inputs of the unsupervised photometric loss at the loss resolution: the scene of ``make_scene`` plus one smooth depth
    map per view ``depths`` [V,B,H,W] (a slanted surface with bumps inside [depth_min, depth_max]; view v's map is what the
    network would predict with view v as the reference)."""
    out = make_scene(B, V, H, W, seed=seed, behind_view=behind_view)
    rng = np.random.default_rng(seed + 77)
    coarse = torch.from_numpy(rng.random((V * B, 1, 4, 5), dtype=np.float32))
    bumps = torch.nn.functional.interpolate(coarse, size=(H, W), mode="bicubic", align_corners=False).reshape(V, B, H, W)
    ramp = torch.linspace(0.0, 1.0, W).view(1, 1, 1, W)
    out["depths"] = (3.2 + 0.8 * ramp + 0.9 * (bumps - 0.5)).contiguous()
    return out


def make_features(B: int, V: int, C: int, h: int, w: int, *, seed: int = 1,
                  scale: float = 0.5) -> torch.Tensor:
    """Feature maps ~ N(0,1)*scale, [V,B,C,h,w] fp32 (hot-path-only timing input)."""
    rng = np.random.default_rng(seed)
    f = rng.standard_normal((V, B, C, h, w), dtype=np.float32) * np.float32(scale)
    return torch.from_numpy(f)


# --------------------------------------------------------------------------
# weights
# --------------------------------------------------------------------------
def _fan_in(shape: Sequence[int], transposed: bool) -> int:
    k = int(np.prod(shape[2:])) if len(shape) > 2 else 1
    cin = shape[0] if transposed else shape[1]
    return max(cin * k, 1)


def make_state_dict(template: Mapping[str, Tuple[int, ...]], *, seed: int = 0,
                    conv_gain: float = 1.6, head_gain: Mapping[str, float] | None = None,
                    transposed_keys: Sequence[str] = ()) -> "OrderedDict[str, torch.Tensor]":
    """Fill a ``{name: shape}`` template (a model's ``state_dict`` key/shape list)
    with deterministic sharpened weights.

    * conv / deconv weights ~ N(0, (gain / sqrt(fan_in))^2)
    * BatchNorm weight ~ U(0.6, 1.4), bias ~ N(0, 0.2), running_mean ~ N(0, 0.2),
      running_var ~ U(0.5, 1.5); ``num_batches_tracked`` = 1
    * conv biases ~ N(0, 0.1); scalar parameters (MVSNet-s ``temp``) = 1
    * ``head_gain`` maps a key substring to an extra multiplier (used to push the
      final 1-channel ``prob`` convs to logit std ~3 so that the softmax peaks).

    The draw order is the template's iteration order, so two models with the same
    key list get identical tensors.
    """
    rng = np.random.default_rng(seed)
    head_gain = dict(head_gain or {})
    out: "OrderedDict[str, torch.Tensor]" = OrderedDict()
    for name, shape in template.items():
        shape = tuple(int(s) for s in shape)
        leaf = name.rsplit(".", 1)[-1]
        if leaf == "num_batches_tracked":
            out[name] = torch.tensor(1, dtype=torch.long)
            continue
        if len(shape) >= 3:  # convolution kernels (2D or 3D)
            transposed = any(name.startswith(k) or k in name for k in transposed_keys)
            std = conv_gain / math.sqrt(_fan_in(shape, transposed))
            for sub, g in head_gain.items():
                if sub in name:
                    std *= g
            arr = rng.standard_normal(shape, dtype=np.float32) * np.float32(std)
        elif leaf == "running_var":
            arr = rng.uniform(0.5, 1.5, size=shape).astype(np.float32)
        elif leaf == "running_mean":
            arr = (rng.standard_normal(shape) * 0.2).astype(np.float32)
        elif leaf == "weight":  # BatchNorm gamma (1-D)
            arr = rng.uniform(0.6, 1.4, size=shape).astype(np.float32)
        elif leaf == "bias":
            arr = (rng.standard_normal(shape) * (0.2 if len(shape) else 0.1)).astype(np.float32)
        elif leaf == "temp":
            arr = np.ones(shape, dtype=np.float32)
        else:
            arr = (rng.standard_normal(shape) * 0.1).astype(np.float32)
        out[name] = torch.from_numpy(np.ascontiguousarray(arr))
    return out


def template_of(module: torch.nn.Module) -> "OrderedDict[str, Tuple[int, ...]]":
    """``{name: shape}`` of a module's state dict, in registration order."""
    return OrderedDict((k, tuple(v.shape)) for k, v in module.state_dict().items())


# gains found by probing the reference on CPU (tests/golden/gen_golden.py prints the
# resulting softmax peak): they give max_d p in the 0.3-0.9 band on make_scene inputs.
SHARPEN = {
    "mvsnet": dict(conv_gain=1.414, head_gain={"feature.": 0.85, "cost_regularization.prob.weight": 10.0}),
    "vis": dict(conv_gain=1.0, head_gain={"final_conv.weight": 2.0}),
    "cvp": dict(conv_gain=1.2, head_gain={"prob0.weight": 12.0}),
}
TRANSPOSED_KEYS = {
    "mvsnet": ("cost_regularization.conv7.0", "cost_regularization.conv9.0", "cost_regularization.conv11.0"),
    "vis": ("dec_blocks",),
    "cvp": ("cost_reg_refine.conv5.0", "cost_reg_refine.conv6.0"),
}


def sharpened_state_dict(arch: str, template: Mapping[str, Tuple[int, ...]], seed: int = 0):
    """``arch`` in {"mvsnet", "vis", "cvp"}."""
    return make_state_dict(template, seed=seed, transposed_keys=TRANSPOSED_KEYS[arch], **SHARPEN[arch])


# ---- training fixtures (shared by tests/golden/gen_golden.py, the oracle tests and the GPU tests) ------------------
TRAIN_PROB_GAIN = 0.3   # keeps the softmax unsaturated under batch-statistics BatchNorm (mean max-prob ~0.5)


def train_state_dict(arch: str, template: Mapping[str, Tuple[int, ...]], seed: int = 0):
    """Sharpened weights for a train()-mode step: ``sharpened_state_dict`` with the `prob` head scaled down."""
    sd = sharpened_state_dict(arch, template, seed=seed)
    for k in list(sd.keys()):
        if k.endswith("cost_regularization.prob.weight") or k.endswith("cost_reg_refine.prob0.weight"):
            sd[k] = sd[k] * TRAIN_PROB_GAIN
    return sd


def train_target(scene, h: int, w: int, seed: int = 11):
    """Seeded ground-truth depth [B,h,w] and validity mask of the supervised loss (models/trainer.py:163-167)."""
    g = torch.Generator().manual_seed(seed)
    dmin, dmax = scene["depth_min"][:, 0].view(-1, 1, 1), scene["depth_max"][:, 0].view(-1, 1, 1)
    gt = dmin + (dmax - dmin) * (0.2 + 0.6 * torch.rand(dmin.shape[0], h, w, generator=g))
    mask = (torch.rand(dmin.shape[0], h, w, generator=g) > 0.1).float()
    return gt, mask


def supervised_loss(depth: torch.Tensor, gt: torch.Tensor, mask: torch.Tensor, depth_min: torch.Tensor, depth_max: torch.Tensor):
    """sum(|d - gt| / interval * mask) / sum(mask), interval = (max - min) / 128 of view 0 (models/trainer.py:163-167)."""
    interval = ((depth_max - depth_min) / 128)[:, 0].view(-1, 1, 1)
    return torch.sum(torch.abs(depth - gt) / interval * mask) / torch.sum(mask)


def supervised_loss_list(depth_list: Sequence[torch.Tensor], gt: torch.Tensor, mask: torch.Tensor, depth_min: torch.Tensor,
                         depth_max: torch.Tensor, reference_frame: int = 0):
    """The supervised loss of models/trainer.py:118-167 over ``depth_est_list``: ground truth and mask are bilinearly
    resized to each estimate (the mask keeps only pixels whose four neighbours are valid), every level has factor 1."""
    import torch.nn.functional as F
    interval = ((depth_max - depth_min) / 128)[:, reference_frame].view(-1, 1, 1)
    loss = 0
    for d in depth_list:
        if d is None:
            continue
        hd, wd = d.shape[1:]
        g = F.interpolate(gt.unsqueeze(1), size=(hd, wd), mode="bilinear", align_corners=False).squeeze(1)
        m = (F.interpolate(mask.unsqueeze(1).float(), size=(hd, wd), mode="bilinear", align_corners=False).squeeze(1) == 1).float()
        loss = loss + torch.sum(torch.abs(d - g) / interval * m) / torch.sum(m)
    return loss


VIS_LOSS_FACTORS = (2, 1, 0.5)   # models/trainer.py:33


def vis_supervised_loss(out, gt: torch.Tensor, mask: torch.Tensor, depth_min: torch.Tensor, depth_max: torch.Tensor, n_views: int):
    """The supervised Vis-MVSNet loss of models/trainer.py:118-206: per stage ``factor * masked L1`` on the fused depth plus
    ``factor / (n - 1) * bayesian_version_loss`` (models/utils.py:110-119) on every pair depth with its log-uncertainty."""
    import torch.nn.functional as F
    interval = ((depth_max - depth_min) / 128)[:, 0].view(-1, 1, 1, 1)
    loss = 0
    for i, d in enumerate(out["depth_est_list"]):
        hd, wd = d.shape[1:]
        g = F.interpolate(gt.unsqueeze(1), size=(hd, wd), mode="bilinear", align_corners=False)
        m = (F.interpolate(mask.unsqueeze(1).float(), size=(hd, wd), mode="bilinear", align_corners=False) == 1).float()
        l1 = torch.abs(d.unsqueeze(1) - g) / interval
        loss = loss + VIS_LOSS_FACTORS[i] * torch.sum(l1 * m) / torch.sum(m)
        for dp, (unc,) in out["depth_pair_list"][i]:
            l1p = torch.abs(dp.squeeze(1).unsqueeze(1) - g) / interval
            loss = loss + VIS_LOSS_FACTORS[i] / (n_views - 1) * (torch.sum((l1p * torch.exp(-unc) + unc) * m) / torch.sum(m)
                                                               + torch.sum(l1p * m) / torch.sum(m))
    return loss


def make_point_cloud_scene(n_pred: int, n_gt: int, *, seed: int = 0, outlier_frac: float = 0.02, dup_frac: float = 0.3,
                           extent: float = 400.0, outliers_only: bool = False) -> Dict[str, np.ndarray]:
    """Inputs of the point-cloud metrics at DTU's millimetre scale: a smooth height-field surface over an ``extent`` square;
    ``gt`` float32 [n_gt,3] samples it with 0.05 mm noise, ``pred`` float32 [n_pred,3] samples it with 0.3 mm noise over 85 % of
    the square (the rest is a hole GT covers alone), ``dup_frac`` of them re-sampled within ~0.1 mm of another (what
    reduce_pts removes) and ``outlier_frac`` of them uniform in the box up to 80 mm off the surface.  ``bb`` [2,3] float64
    encloses the surface with a margin.  ``outliers_only``: every prediction instead lies 30-70 mm above a flat GT patch (the
    bounded search's worst case)."""
    rng = np.random.default_rng(seed)
    height = lambda x, y: 40.0 * np.sin(x / 70.0) * np.cos(y / 90.0) + 0.05 * x
    gxy = rng.uniform(0.0, extent, size=(n_gt, 2))
    if outliers_only:
        gt = np.concatenate((gxy, rng.normal(0.0, 0.05, (n_gt, 1))), axis=1)
        pxy = rng.uniform(0.0, extent, size=(n_pred, 2))
        pred = np.concatenate((pxy, rng.uniform(30.0, 70.0, (n_pred, 1))), axis=1)
    else:
        gt = np.concatenate((gxy, (height(gxy[:, 0], gxy[:, 1]) + rng.normal(0.0, 0.05, n_gt))[:, None]), axis=1)
        n_out = int(n_pred * outlier_frac)
        n_dup = int(n_pred * dup_frac)
        n_surf = n_pred - n_out - n_dup
        pxy = rng.uniform(0.0, extent, size=(n_surf, 2))
        pxy[:, 0] = pxy[:, 0] * 0.85                                  # the last 15 % along x: a hole in the prediction
        surf = np.concatenate((pxy, height(pxy[:, 0], pxy[:, 1])[:, None]), axis=1) + rng.normal(0.0, 0.3, (n_surf, 3))
        dup = surf[rng.integers(0, max(n_surf, 1), n_dup)] + rng.normal(0.0, 0.06, (n_dup, 3))
        out = rng.uniform([0.0, 0.0, -80.0], [extent, extent, 120.0], size=(n_out, 3))
        pred = np.concatenate((surf, dup, out))[rng.permutation(n_pred)]
    bb = np.array([[-20.0, -20.0, -100.0], [extent + 20.0, extent + 20.0, 140.0]])
    return {"pred": pred.astype(np.float32), "gt": gt.astype(np.float32), "bb": bb}


def make_yfcc_fusion_scene(V: int, H: int, W: int, *, seed: int = 0, overlap: str = "all", k_overlap: int = 3,
                           perturb: float = 0.003, outlier_view: int = 1, mask_frac: float = 0.02,
                           spacing: float = 0.25) -> Dict[str, object]:
    """Inputs of the COLMAP-style fusion on an "in the wild" subset: ``make_fusion_scene``'s rig and tilted plane, but every view
    has its own size (ragged: height and width each 70-100 % of H, W, own intrinsics, focal 0.9 w), view ``outlier_view`` a
    block of gross outliers (x 1.25), every view ``mask_frac`` masked (0) pixels and one masked rectangle.  ``overlap`` picks
    the graph COLMAP would take from a sparse model: "all" (every other view, nearest camera centre first, ties by index),
    "knn" (the ``k_overlap`` nearest views only: sparse and not symmetric in general) or "chain" (v-1 and v+1).  Returns
    ``depths``, ``colors`` (uint8 [h,w,3]), ``K``, ``R`` [V,3,3], ``t`` [V,3,1] (float32 tensors) and ``overlap`` (V lists)."""
    rng = np.random.default_rng(seed)
    n = np.array([0.10, -0.06, 1.0])
    n = n / np.linalg.norm(n)
    c0 = 4.0 * n[2]
    g = int(math.ceil(math.sqrt(V)))
    K, R, t, depths, colors, centres = [], [], [], [], [], []
    for v in range(V):
        h, w = int(round(H * rng.uniform(0.7, 1.0))), int(round(W * rng.uniform(0.7, 1.0)))
        f = 0.9 * w
        Kv = np.array([[f, 0.0, w / 2.0 + rng.uniform(-0.5, 0.5)], [0.0, f * rng.uniform(0.98, 1.02), h / 2.0 + rng.uniform(-0.5, 0.5)],
                       [0.0, 0.0, 1.0]])
        gx, gy = v % g - (g - 1) / 2.0, v // g - (g - 1) / 2.0
        c = np.array([gx * spacing, gy * spacing, 0.0]) + rng.normal(0.0, 0.02 * spacing, 3)
        ay, ax = -0.25 * gx * spacing / 4.0 + rng.normal(0.0, 0.01), 0.25 * gy * spacing / 4.0 + rng.normal(0.0, 0.01)
        cy, sy, cx, sx = math.cos(ay), math.sin(ay), math.cos(ax), math.sin(ax)
        Rv = np.array([[1.0, 0.0, 0.0], [0.0, cx, -sx], [0.0, sx, cx]]) @ np.array([[cy, 0.0, sy], [0.0, 1.0, 0.0], [-sy, 0.0, cy]])
        tv = -Rv @ c
        ys, xs = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
        p = np.stack((xs, ys, np.ones_like(xs)), axis=-1).reshape(-1, 3)
        ray = p @ np.linalg.inv(Kv).T @ Rv
        d = ((c0 - n @ c) / (ray @ n)).reshape(h, w)
        X = c + d.reshape(-1, 1) * ray
        col = np.stack((128 + 100 * np.sin(3.1 * X[:, 0]), 128 + 100 * np.sin(2.3 * X[:, 1] + 1.0),
                        128 + 100 * np.cos(1.7 * (X[:, 0] + X[:, 1]))), axis=-1).reshape(h, w, 3) + rng.normal(0.0, 2.0, (h, w, 3))
        coarse = torch.from_numpy(rng.standard_normal((1, 1, max(h // 8, 2), max(w // 8, 2))))
        bump = torch.nn.functional.interpolate(coarse, size=(h, w), mode="bilinear", align_corners=False)[0, 0].numpy()
        d = d * (1.0 + perturb * np.tanh(bump))
        if v == outlier_view:
            d[h // 4:h // 2, w // 3:w // 2] *= 1.25
        d[rng.random((h, w)) < mask_frac] = 0.0
        r0, c0_ = int(rng.integers(0, max(h - 4, 1))), int(rng.integers(0, max(w - 6, 1)))
        d[r0:r0 + 3, c0_:c0_ + 5] = 0.0
        K.append(Kv); R.append(Rv); t.append(tv.reshape(3, 1)); centres.append(c)
        depths.append(torch.from_numpy(d.astype(np.float32)).contiguous())
        colors.append(torch.from_numpy(np.clip(np.rint(col), 0, 255).astype(np.uint8)).contiguous())
    cen = np.stack(centres)
    dist = np.linalg.norm(cen[:, None] - cen[None], axis=-1)
    lists = []
    for v in range(V):
        others = sorted((u for u in range(V) if u != v), key=lambda u: (dist[v, u], u))
        if overlap == "all":
            lists.append(others)
        elif overlap == "knn":
            lists.append(others[:k_overlap])
        elif overlap == "chain":
            lists.append([u for u in (v - 1, v + 1) if 0 <= u < V])
        else:
            raise ValueError(f"make_yfcc_fusion_scene: unknown overlap {overlap!r}")
    f32 = lambda a: torch.from_numpy(np.stack(a).astype(np.float32))
    return {"depths": depths, "colors": colors, "K": f32(K), "R": f32(R), "t": f32(t), "overlap": lists}


def make_permuted_yfcc_fusion_scene(V: int, H: int, W: int, *, perm_seed: int = 0, **kw) -> Dict[str, object]:
    """``make_yfcc_fusion_scene(V, H, W, **kw)`` with the view order shuffled by a seeded permutation, so that index neighbours are
    not spatial neighbours (an unordered photo collection): view k of the result is view ``perm[k]`` of the grid rig.  The
    ``overlap`` lists are renumbered with the views; ``perm`` is returned with the scene."""
    sc = make_yfcc_fusion_scene(V, H, W, **kw)
    perm = np.random.default_rng(perm_seed).permutation(V)
    inv = np.empty(V, dtype=np.int64)
    inv[perm] = np.arange(V)
    idx = torch.from_numpy(perm)
    return {"depths": [sc["depths"][p] for p in perm], "colors": [sc["colors"][p] for p in perm], "K": sc["K"][idx].contiguous(),
            "R": sc["R"][idx].contiguous(), "t": sc["t"][idx].contiguous(),
            "overlap": [[int(inv[u]) for u in sc["overlap"][p]] for p in perm], "perm": perm}


def _pm_texture(X: np.ndarray, freqs: np.ndarray, phases: np.ndarray) -> np.ndarray:
    """Procedural colour in [0,1] of world points X [N,3]: per channel tanh of a sum of 3-D sinusoids (freqs [3,k,3], phases
    [3,k]), so every view sees the same surface pattern."""
    return np.stack([0.5 + 0.45 * np.tanh((np.sin(X @ freqs[c].T + phases[c][None])).sum(1) / math.sqrt(freqs.shape[1] / 2.0))
                     for c in range(3)], axis=0)


def make_patch_match_scene(V: int, H: int, W: int, *, seed: int = 0, spacing: float = 0.4, noise: float = 0.002
                           ) -> Dict[str, object]:
    """A photo-consistent scene for the PatchMatch stereo with ground truth.  A tilted background plane (depth about 5) and an
    occluding sphere in front (depth about 2.7-3.5), textured by ``_pm_texture`` in world coordinates except an untextured disc on
    the plane (constant grey, radius 1); V pinhole cameras on a ragged grid (``spacing`` apart, jittered, each looking at a jittered point
    of the scene), all H x W with focal 0.9 W; colours averaged over 2 x 2 samples per pixel; per-view gain and bias and Gaussian noise (``noise``) on the [0,1] image.

    Returns ``imgs`` [V,3,H,W] in [0,1], ``K``, ``R`` [V,3,3], ``t`` [V,3,1], ``depth_min``, ``depth_max`` [V] (0.8 x / 1.25 x
    the view's true range), ``src`` (per view: every other view, nearest camera centre first), the ground truth ``depth`` [V,H,W]
    and ``normal`` [V,H,W,3] (camera frame, facing the camera), ``untextured`` [V,H,W] bool (pixels whose 11 x 11 window lies
    wholly on the disc) and ``vis`` [V,H,W] int (the
    number of other views that see the pixel's point unoccluded inside their image) -- float32 / bool / int64 tensors."""
    rng = np.random.default_rng(seed)
    pn = np.array([0.2, -0.15, -1.0])
    pn /= np.linalg.norm(pn)
    p0 = np.array([0.0, 0.0, 5.0])
    sc, sr = np.array([0.3, 0.15, 3.6]), 0.8
    u_ax = np.cross(pn, [0.0, 1.0, 0.0]); u_ax /= np.linalg.norm(u_ax)
    disc = p0 + 1.5 * u_ax + 1.0 * np.cross(pn, u_ax)           # centre of the untextured disc on the plane, radius 1
    mags = rng.uniform(12.0, 36.0, (3, 10))
    dirs = rng.standard_normal((3, 10, 3))
    freqs = dirs / np.linalg.norm(dirs, axis=-1, keepdims=True) * mags[..., None]
    phases = rng.uniform(0.0, 2.0 * math.pi, (3, 10))
    g = int(math.ceil(math.sqrt(V)))
    Ks, Rs, ts, cs = [], [], [], []
    for v in range(V):
        f = 0.9 * W
        Ks.append(np.array([[f, 0.0, W / 2.0 + rng.uniform(-1, 1)], [0.0, f * rng.uniform(0.98, 1.02), H / 2.0 + rng.uniform(-1, 1)],
                            [0.0, 0.0, 1.0]]))
        c = np.array([(v % g - (g - 1) / 2.0) * spacing, (v // g - (g - 1) / 2.0) * spacing, 0.0]) + rng.normal(0.0, 0.15 * spacing, 3)
        z = np.array([0.0, 0.0, 4.5]) + rng.normal(0.0, 0.3, 3) - c
        z /= np.linalg.norm(z)
        x = np.cross([0.0, 1.0, 0.0], z); x /= np.linalg.norm(x)
        Rv = np.stack([x, np.cross(z, x), z])
        Rs.append(Rv); ts.append(-Rv @ c); cs.append(c)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    pix = np.stack((xs, ys, np.ones_like(xs)), axis=-1).reshape(-1, 3)
    depth, normal, world, imgs, untex = [], [], [], [], []
    for v in range(V):
        r = pix @ np.linalg.inv(Ks[v]).T @ Rs[v]                      # world ray per pixel with camera-frame z = 1
        c = cs[v]
        lam_p = (pn @ (p0 - c)) / (r @ pn)
        oc = c - sc
        a, b, cc = (r * r).sum(1), 2.0 * (r @ oc), oc @ oc - sr * sr
        disc_ = b * b - 4 * a * cc
        lam_s = np.where(disc_ >= 0, (-b - np.sqrt(np.maximum(disc_, 0.0))) / (2 * a), np.inf)
        hit_s = (lam_s > 0) & (lam_s < lam_p)
        lam = np.where(hit_s, lam_s, lam_p)
        X = c + lam[:, None] * r
        nw = np.where(hit_s[:, None], (X - sc) / sr, pn[None])
        nc = nw @ Rs[v].T
        nc = np.where(((nc * (pix @ np.linalg.inv(Ks[v]).T)).sum(1) > 0)[:, None], -nc, nc)
        flat = ~hit_s & (np.linalg.norm(X - disc, axis=1) < 1.0)
        col = np.zeros((3, H * W))
        for sy, sx in ((-0.25, -0.25), (-0.25, 0.25), (0.25, -0.25), (0.25, 0.25)):     # 2 x 2 supersampling of the texture
            rs = (pix + np.array([sx, sy, 0.0])) @ np.linalg.inv(Ks[v]).T @ Rs[v]
            lp = (pn @ (p0 - c)) / (rs @ pn)
            bs = 2.0 * (rs @ oc)
            ds_ = bs * bs - 4 * (rs * rs).sum(1) * cc
            ls = np.where(ds_ >= 0, (-bs - np.sqrt(np.maximum(ds_, 0.0))) / (2 * (rs * rs).sum(1)), np.inf)
            ls = np.where((ls > 0) & (ls < lp), ls, lp)
            Xs = c + ls[:, None] * rs
            col += 0.25 * np.where((np.linalg.norm(Xs - disc, axis=1) < 1.0)[None], 0.5, _pm_texture(Xs, freqs, phases))
        gain, bias = rng.uniform(0.75, 1.15), rng.uniform(-0.05, 0.08)
        img = np.clip(gain * col + bias + rng.normal(0.0, noise, col.shape), 0.0, 1.0)
        depth.append(lam.reshape(H, W)); normal.append(nc.reshape(H, W, 3)); world.append(X)
        # untextured for a window matcher: the whole 11 x 11 window lies on the disc (erosion by 5 pixels)
        fl = flat.reshape(H, W)
        er = fl.copy()
        for dy in range(-5, 6):
            for dx in range(-5, 6):
                er &= np.roll(fl, (dy, dx), axis=(0, 1))
        er[:5] = er[-5:] = False
        er[:, :5] = er[:, -5:] = False
        imgs.append(img.reshape(3, H, W)); untex.append(er)
    vis = np.zeros((V, H * W), dtype=np.int64)
    for v in range(V):
        for s in range(V):
            if s == v:
                continue
            y = (world[v] @ Rs[s].T + ts[s]) @ Ks[s].T
            ok = y[:, 2] > 0
            u, w_ = y[:, 0] / np.where(ok, y[:, 2], 1.0), y[:, 1] / np.where(ok, y[:, 2], 1.0)
            qx, qy = np.floor(u + 0.5).astype(np.int64), np.floor(w_ + 0.5).astype(np.int64)
            ok &= (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
            ds = depth[s][np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)]
            vis[v] += ok & (np.abs(ds - y[:, 2]) <= 0.01 * y[:, 2])
    cen = np.stack(cs)
    src = [sorted((u for u in range(V) if u != v), key=lambda u: (float(np.linalg.norm(cen[u] - cen[v])), u)) for v in range(V)]
    f32 = lambda a: torch.from_numpy(np.stack(a).astype(np.float32))
    dep = np.stack(depth)
    return {"imgs": f32(imgs), "K": f32(Ks), "R": f32(Rs), "t": f32([t.reshape(3, 1) for t in ts]),
            "depth_min": torch.from_numpy((0.8 * dep.reshape(V, -1).min(1)).astype(np.float32)),
            "depth_max": torch.from_numpy((1.25 * dep.reshape(V, -1).max(1)).astype(np.float32)),
            "src": src, "depth": f32(depth), "normal": f32(normal), "untextured": torch.from_numpy(np.stack(untex)),
            "vis": torch.from_numpy(vis.reshape(V, H, W))}


def make_normal_fusion_scene(V: int, H: int, W: int, *, seed: int = 0, overlap: str = "all", k_overlap: int = 3,
                             jitter_deg: float = 2.5, rot_view: int = 1, rot_deg: float = 25.0, rot_frac: float = 0.5,
                             outlier_view: int = 0, mask_frac: float = 0.02, spacing: float = 0.4) -> Dict[str, object]:
    """Inputs of the COLMAP-style fusion with normal maps, with ground truth: ``make_patch_match_scene``'s tilted plane and
    occluding sphere seen by V cameras, all H x W.  The depth maps are the true depths; the normal maps (camera frame, unit) are
    the true normals with a Gaussian tangent jitter (``jitter_deg`` per tangent axis, seeded) everywhere.  In view ``rot_view`` a
    central block (``rot_frac`` of the height and of the width) has its normals turned by ``rot_deg`` about a tangent axis while
    its depths stay true, so the normal test alone can refuse those pixels.  View ``outlier_view`` has a block of gross depth
    outliers (x 1.25); every view has ``mask_frac`` filtered pixels and one filtered rectangle (depth 0, normal 0).  ``overlap``
    as in ``make_yfcc_fusion_scene``: "all" (nearest camera centre first), "knn" or "chain".

    Returns ``depths`` V x float32 [H,W], ``normals`` V x float32 [H,W,3], ``colors`` V x uint8 [H,W,3] (the image x 255
    truncated), ``K``, ``R`` [V,3,3], ``t`` [V,3,1], ``overlap`` (V lists), and the ground truth ``depth_gt`` [V,H,W] and
    ``normal_world`` [V,H,W,3] (the true world normal at every pixel, facing its camera), ``rotated`` [V,H,W] bool."""
    pm = make_patch_match_scene(V, H, W, seed=seed, spacing=spacing)
    rng = np.random.default_rng([seed, 0x6E6F726D])
    R = pm["R"].numpy().astype(np.float64)
    n_true = pm["normal"].numpy().astype(np.float64)                       # [V,H,W,3] camera frame
    depth_gt = pm["depth"].numpy().astype(np.float64)
    normal_world = np.einsum("vji,vhwj->vhwi", R, n_true)                    # R^T n
    sig = math.radians(jitter_deg)
    depths, normals, colors, rotated = [], [], [], []
    for v in range(V):
        n = n_true[v]
        g = rng.standard_normal((H, W, 3))
        nj = n + sig * (g - (g * n).sum(-1, keepdims=True) * n)
        nj /= np.linalg.norm(nj, axis=-1, keepdims=True)
        rot = np.zeros((H, W), dtype=bool)
        if v == rot_view % V:
            bh, bw = max(int(round(H * rot_frac)), 1), max(int(round(W * rot_frac)), 1)
            r0, c0 = (H - bh) // 2, (W - bw) // 2
            rot[r0:r0 + bh, c0:c0 + bw] = True
            k = np.cross(nj, np.array([0.0, 1.0, 0.0]))
            k /= np.linalg.norm(k, axis=-1, keepdims=True)                   # a tangent axis: the turn is rot_deg exactly
            th = math.radians(rot_deg)
            turned = nj * math.cos(th) + np.cross(k, nj) * math.sin(th)
            nj = np.where(rot[..., None], turned, nj)
        d = depth_gt[v].copy()
        if v == outlier_view % V:
            d[H // 8:H // 4, W // 8:W // 3] *= 1.25
        gone = rng.random((H, W)) < mask_frac
        r0, c0 = int(rng.integers(0, max(H - 4, 1))), int(rng.integers(0, max(W - 6, 1)))
        gone[r0:r0 + 3, c0:c0 + 5] = True
        d[gone] = 0.0
        nj[gone] = 0.0
        depths.append(torch.from_numpy(d.astype(np.float32)).contiguous())
        normals.append(torch.from_numpy(nj.astype(np.float32)).contiguous())
        colors.append(pm["imgs"][v].mul(255).byte().permute(1, 2, 0).contiguous())
        rotated.append(rot)
    lists = []
    for v in range(V):
        others = list(pm["src"][v])
        if overlap == "all":
            lists.append(others)
        elif overlap == "knn":
            lists.append(others[:k_overlap])
        elif overlap == "chain":
            lists.append([u for u in (v - 1, v + 1) if 0 <= u < V])
        else:
            raise ValueError(f"make_normal_fusion_scene: unknown overlap {overlap!r}")
    return {"depths": depths, "normals": normals, "colors": colors, "K": pm["K"], "R": pm["R"], "t": pm["t"], "overlap": lists,
            "depth_gt": torch.from_numpy(depth_gt.astype(np.float32)), "normal_world": torch.from_numpy(normal_world.astype(np.float32)),
            "rotated": torch.from_numpy(np.stack(rotated))}


def patch_match_batches(scene: Mapping[str, object], names: Sequence[str] = None, max_src: int = None):
    """Dataloader batches of a ``make_patch_match_scene`` scene, shaped like the YFCC loader's (batch size 1): per reference view
    v, ``imgs`` [1,1+S,3,H,W], ``K``, ``R`` [1,1+S,3,3], ``t`` [1,1+S,3,1], ``depth_min``, ``depth_max`` [1,1+S], ``filename`` [name]
    and ``src_filenames`` [[name] per source], sources = ``scene["src"][v]`` (the first ``max_src``)."""
    V = scene["imgs"].shape[0]
    names = [f"{v:08d}" for v in range(V)] if names is None else list(names)
    out = []
    for v in range(V):
        ids = [v] + list(scene["src"][v])[:max_src]
        out.append({"imgs": scene["imgs"][ids][None], "K": scene["K"][ids][None], "R": scene["R"][ids][None],
                    "t": scene["t"][ids][None], "depth_min": scene["depth_min"][ids][None], "depth_max": scene["depth_max"][ids][None],
                    "filename": [names[v]], "src_filenames": [[names[u]] for u in ids[1:]]})
    return out
