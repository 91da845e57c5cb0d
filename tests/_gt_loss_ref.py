"""numpy / torch restatement of the loss reductions and depth-map scores, the yardstick of
csrc/depth_gt.hip: the tap rule that equals ``F.interpolate(mode="bilinear", align_corners=False)`` for integer ratios, the four
kinds of term with their gradients, and the five metric functions behind a bilinear upsampling with torch's fp32 index rule.
Sums are fp64; what the kernels do in fp32 per pixel (the resized ground truth, the per-pixel loss) is fp32 here too."""
from __future__ import annotations

import numpy as np

GT_PLAIN, GT_BAYES, L_PLAIN, L_BAYES = 0, 1, 2, 3
MAX_TERMS, MAX_THRESH = 32, 4


# ---- ground truth at the depth map's size ----------------------------------------------------------------------------------------
def taps(r: int, n: int) -> np.ndarray:
    """[n, k] source indices of the taps of output index i for the integer ratio r: one for an odd ratio (weight 1), two for an
    even one (weight 0.5 each)."""
    i = np.arange(n)
    if r % 2:
        return (r * i + (r - 1) // 2)[:, None]
    first = r * i + r // 2 - 1
    return np.stack([first, first + 1], axis=1)


def gt_down(gt: np.ndarray, mask: np.ndarray, h: int, w: int, dtype=np.float32):
    """gt fp32 [b,H,W], mask [b,H,W] (bool, or numbers holding 0 / 1) -> (gt_down fp32 [b,h,w], m bool [b,h,w]); m is True iff
    every tap used is valid.  gt_down = 0.5 (0.5 a + 0.5 b) + 0.5 (0.5 c + 0.5 d) in that association, in ``dtype``."""
    b, H, W = gt.shape
    if H % h or W % w:
        raise ValueError("non-integer ratio")
    ty, tx = taps(H // h, h), taps(W // w, w)
    valid = np.asarray(mask) != 0
    gt = gt.astype(dtype)
    half = dtype(0.5)

    def row(yi):                                        # the horizontal taps of source rows yi [h] -> [b,h,w]
        g = gt[:, yi][:, :, tx]                         # [b,h,w,k]
        v = valid[:, yi][:, :, tx]
        if tx.shape[1] == 2:
            return half * g[..., 0] + half * g[..., 1], v[..., 0] & v[..., 1]
        return g[..., 0], v[..., 0]

    r0, m = row(ty[:, 0])
    if ty.shape[1] == 2:
        r1, m1 = row(ty[:, 1])
        return (half * r0 + half * r1).astype(dtype), m & m1
    return r0.astype(dtype), m


def invalid_taps(mask: np.ndarray, h: int, w: int) -> np.ndarray:
    """Number of invalid taps per output pixel [b,h,w] (the fixture wants every count from 1 to 3 present)."""
    b, H, W = mask.shape
    ty, tx = taps(H // h, h), taps(W // w, w)
    bad = (np.asarray(mask) == 0)
    return bad[:, ty[:, :, None, None], tx[None, None, :, :]].sum(axis=(2, 4))


# ---- terms ---------------------------------------------------------------------------------------------------------------------------
def pixel_loss(kind, a, gt=None, mask=None, interval=None, dtype=np.float32):
    """-> (l, m bool, sign / interval) with the shape of ``a`` flattened to [b,h,w] for the ground-truth kinds; the arithmetic per
    pixel is done in ``dtype`` (fp32: what the kernel does; fp64: what the fixture's expectations were computed in)."""
    if kind in (GT_PLAIN, GT_BAYES):
        b, h, w = a.shape[0], a.shape[-2], a.shape[-1]
        d = a.reshape(b, h, w).astype(dtype)
        g, m = gt_down(gt.reshape(b, *gt.shape[-2:]), np.asarray(mask).reshape(b, *gt.shape[-2:]), h, w, dtype)
        iv = interval.reshape(b, 1, 1).astype(dtype)
        diff = d - g
        return (np.abs(diff) / iv).astype(dtype), m, (np.sign(diff) / iv).astype(dtype)
    return a.astype(dtype), np.asarray(mask).reshape(a.shape) != 0, None


def term(kind, a, mask, u=None, gt=None, interval=None, dtype=np.float32):
    """-> dict(value, sums = (S_l, S_u, C), norm) in fp64 (NaN / inf for a GT_PLAIN term with an empty mask)."""
    l, m, _ = pixel_loss(kind, a, gt, mask, interval, dtype)
    l64, m64 = l.astype(np.float64), m.astype(np.float64)
    Sl, Cn = float((l64 * m64).sum()), float(m64.sum())
    bayes = kind in (GT_BAYES, L_BAYES)
    Su = 0.0
    if bayes:
        u32 = u.reshape(l.shape).astype(dtype)
        Su = float(((l * np.exp(-u32) + u32).astype(np.float64) * m64).sum())
    with np.errstate(divide="ignore", invalid="ignore"):
        if kind == GT_PLAIN:
            value, norm = np.float64(Sl) / np.float64(Cn), np.float64(1.0) / np.float64(Cn)
        else:
            tot = Su + Sl if bayes else Sl
            value, norm = (tot / Cn, 1.0 / Cn) if Cn != 0 else (tot, 1.0)
    return dict(value=float(value), sums=(Sl, Su, Cn), norm=float(norm))


def term_grads(kind, factor, g, a, mask, u=None, gt=None, interval=None, dtype=np.float32):
    """Gradients of g * factor * term to ``a`` (the depth map or the given loss) and ``u`` (None for the plain kinds), fp64, in the
    shape of ``a`` / ``u``."""
    l, m, sgn = pixel_loss(kind, a, gt, mask, interval, dtype)
    n = term(kind, a, mask, u, gt, interval, dtype)["norm"]
    coef = np.float64(g) * np.float64(factor) * np.float64(n)
    m64, l64 = m.astype(np.float64), l.astype(np.float64)
    bayes = kind in (GT_BAYES, L_BAYES)
    e = np.exp(-u.reshape(l.shape).astype(np.float64)) if bayes else None
    wa = (e + 1.0) if bayes else np.ones_like(l64)
    if sgn is not None:
        wa = wa * sgn.astype(np.float64)
    da = (coef * m64 * wa).reshape(a.shape)
    du = (coef * m64 * (1.0 - l64 * e)).reshape(u.shape) if bayes else None
    return da, du


# ---- scores ----------------------------------------------------------------------------------------------------------------------
def _src_index(n_in: int, n_out: int):
    """torch's upsample_bilinear2d index rule (align_corners=False) in fp32 -> (i0, i1, l0, l1), each [n_out]."""
    scale = np.float32(n_in) / np.float32(n_out)
    s = scale * (np.arange(n_out, dtype=np.float32) + np.float32(0.5)) - np.float32(0.5)
    s = np.maximum(s, np.float32(0)).astype(np.float32)
    i0 = np.minimum(s.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = (s - i0.astype(np.float32)).astype(np.float32)
    return i0, i1, (np.float32(1) - l1).astype(np.float32), l1


def upsample(est: np.ndarray, H: int, W: int) -> np.ndarray:
    """est fp32 [b,h,w] -> [b,H,W] as F.interpolate(mode="bilinear", align_corners=False) on fp32."""
    est = est.astype(np.float32)
    y0, y1, ly0, ly1 = _src_index(est.shape[1], H)
    x0, x1, lx0, lx1 = _src_index(est.shape[2], W)
    r0, r1 = est[:, y0], est[:, y1]
    top = lx0 * r0[:, :, x0] + lx1 * r0[:, :, x1]
    bot = lx0 * r1[:, :, x0] + lx1 * r1[:, :, x1]
    return (ly0[None, :, None] * top + ly1[None, :, None] * bot).astype(np.float32)


def metric_pixels(est, gt, mask, step=None):
    """-> per image: (|e - g|, |e - g| / g, (e - g)^2 / g, max(e / g, g / e)) over the valid pixels, fp32 like the kernel's."""
    b, H, W = gt.shape
    up = upsample(est.reshape(b, *est.shape[-2:]), H, W)
    st = np.ones(b, np.float32) if step is None else step.astype(np.float32)
    out = []
    for i in range(b):
        valid = mask[i] != 0 if mask.dtype == np.bool_ or mask.dtype == np.uint8 else mask[i] > 0.5
        e, g = (up[i] / st[i])[valid], (gt[i].astype(np.float32) / st[i])[valid]
        ad = np.abs(e - g)
        with np.errstate(divide="ignore", invalid="ignore"):
            out.append((ad, ad / g, (e - g) * (e - g) / g, np.maximum(e / g, g / e)))
    return out


def metrics(est, gt, mask, step=None, thresholds=(1, 3), rel_thresholds=()):
    """-> dict(sums fp64 [b, 4 + 2 * 4], EPE, thres [..], Rel, SqRel, rel_thres [..] (batch means), per_image (the same, [b, ...]))."""
    px = metric_pixels(est, gt, mask, step)
    b = len(px)
    sums = np.zeros((b, 4 + 2 * MAX_THRESH))
    for i, (ad, rel, sq, ratio) in enumerate(px):
        sums[i, 0], sums[i, 1] = ad.size, ad.astype(np.float64).sum()
        sums[i, 2 + MAX_THRESH], sums[i, 3 + MAX_THRESH] = rel.astype(np.float64).sum(), sq.astype(np.float64).sum()
        for k, t in enumerate(thresholds):
            sums[i, 2 + k] = (ad > np.float32(t)).sum()
        for k, r in enumerate(rel_thresholds):
            sums[i, 4 + MAX_THRESH + k] = (ratio > np.float32(r)).sum()
    with np.errstate(divide="ignore", invalid="ignore"):
        C = sums[:, :1]
        per = dict(EPE=sums[:, 1] / C[:, 0], thres=sums[:, 2:2 + len(thresholds)] / C, Rel=sums[:, 2 + MAX_THRESH] / C[:, 0],
                   SqRel=sums[:, 3 + MAX_THRESH] / C[:, 0], rel_thres=1.0 - sums[:, 4 + MAX_THRESH:4 + MAX_THRESH + len(rel_thresholds)] / C)
    out = {k: v.mean(axis=0) for k, v in per.items()}
    out["per_image"], out["sums"] = per, sums
    return out


def threshold_margin(est, gt, mask, step, thresholds, rel_thresholds) -> float:
    """Smallest relative distance of a valid pixel's |e - g| (ratio) from an absolute (ratio) threshold."""
    best = np.inf
    for ad, _, _, ratio in metric_pixels(est, gt, mask, step):
        for t in thresholds:
            if ad.size:
                best = min(best, float(np.abs(ad.astype(np.float64) - t).min() / t))
        for r in rel_thresholds:
            if ratio.size:
                best = min(best, float(np.abs(ratio.astype(np.float64) - r).min() / r))
    return best


# ---- the fixture's term table (tests/golden/gtloss_tiny.npz) ---------------------------------------------------------------------
SCALES = ("s1", "s2", "s4", "s3", "s21")


def fixture_terms(z):
    """All four kinds in one table of 20 terms: per scale a GT_PLAIN term and two GT_BAYES pair terms, then the L kinds with the
    float and the bool mask, and an L_BAYES term with an empty mask.  -> list of dict(kind, factor, a, mask, u, gt, interval, want)
    where ``want`` is the fixture's fp64 expectation of the term."""
    terms = []
    for k, s in enumerate(SCALES):
        common = dict(gt=z["gt"], mask=z["gt_mask"], interval=z["interval"])
        terms.append(dict(kind=GT_PLAIN, factor=(2.0, 1.0, 0.5, 1.0, 0.25)[k], a=z[f"{s}_d"], u=None, want=float(z[f"{s}_plain"]), **common))
        for j in range(2):
            terms.append(dict(kind=GT_BAYES, factor=0.5 + 0.25 * j, a=z[f"{s}_p{j}_d"], u=z[f"{s}_p{j}_u"], want=float(z[f"{s}_p{j}_bayes"]),
                              **common))
    none = dict(gt=None, interval=None)
    terms.append(dict(kind=L_PLAIN, factor=1.0, a=z["l"], mask=z["l_mask_f"], u=None, want=float(z["l_plain_f"]), **none))
    terms.append(dict(kind=L_PLAIN, factor=0.5, a=z["l"], mask=z["l_mask_b"], u=None, want=float(z["l_plain_b"]), **none))
    terms.append(dict(kind=L_BAYES, factor=0.75, a=z["l"], mask=z["l_mask_f"], u=z["l_u"], want=float(z["l_bayes_f"]), **none))
    terms.append(dict(kind=L_BAYES, factor=0.125, a=z["l"], mask=z["l_mask_b"], u=z["l_u"], want=float(z["l_bayes_b"]), **none))
    terms.append(dict(kind=L_BAYES, factor=1.5, a=z["l"], mask=np.zeros_like(z["l_mask_f"]), u=z["l_u"], want=float(z["l_bayes_empty"]), **none))
    return terms


def term_of(t, dtype=np.float32):
    return term(t["kind"], t["a"], t["mask"], t["u"], t["gt"], t["interval"], dtype)


def grads_of(t, g=1.0, dtype=np.float32):
    return term_grads(t["kind"], t["factor"], g, t["a"], t["mask"], t["u"], t["gt"], t["interval"], dtype)
