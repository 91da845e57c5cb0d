"""Plain float64 reference of ``pscv_warp_cost_bwd`` (csrc/warp_bwd.hip), independent of the kernels' code.

It takes what the C ABI takes -- camera blocks [n_src,B,18], depth planes [B,D] or [B,D,h,w], channels-last features and the
upstream gradient -- and restates the documented semantics of ``sweep_index`` in float64:

* PROJ   ``q = rot p d + trans`` on integer pixel centres (rot = block[0:9], trans = block[9:12]),
* HOMOG  ``q = A p - (Bm p) / (d + 1e-9)`` on half-pixel centres (A = block[0:9], Bm = block[9:18]), divisor clamped at 1e-9,
* ``q_z <= 0`` sends the sample to (-10, -10),
* the index scale (PROJ 1, HOMOG (size - 1) / size) and the clamp implied by the reference's grid clamp
  (PROJ [-4.5, 5.5] (size - 1), HOMOG [-0.05, 1.05] (size - 1)), as set in ``pscv_warp_cost_bwd``.

Sampling is ``F.grid_sample`` (bilinear, zeros, align_corners=True) in float64, the five cost statistics follow the oracle's
formulas, and the gradients come from autograd.  ``tap_scatter`` restates the bilinear scatter by hand (it does not go through
grid_sample), which gives the per-texel tap counts and absolute sums the error-bound tests need, and a second, independent route
to ``dsrc`` that tests/test_warp_bwd_ref_cpu.py holds against autograd.

The same pieces give the FORWARD volume of ``pscv_warp_cost_rows`` (``forward``; ``variance_partial`` / ``variance_finish``;
``positions`` with ``ref_y0``), and ``fragile`` marks the samples whose fp32 evaluation may sit on the other side of q_z = 0:
tests/test_gpu_warp_fwd.py compares every forward kernel family with it, tests/test_warp_fwd_ref_cpu.py pins it to the oracles.
"""
import math

import torch
import torch.nn.functional as F

COSTS = ("variance", "variance_cvp", "softmin", "groupcorr", "warp_only")
GEOMS = ("proj", "homog")


def _pixels(geom, ref_hw, ref_y0):
    """Homogeneous reference pixel coordinates [3,hw] float64: integer centres (PROJ) or half-pixel centres (HOMOG); row y of the
    slab is row y + ref_y0 of the whole grid (WarpArgs::ref_y0)."""
    h, w = int(ref_hw[0]), int(ref_hw[1])
    off = 0.5 if geom == "homog" else 0.0
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float64) + (off + int(ref_y0)), torch.arange(w, dtype=torch.float64) + off, indexing="ij")
    return torch.stack((xx.reshape(-1), yy.reshape(-1), torch.ones(h * w, dtype=torch.float64)))


def positions(cams, depth, geom, ref_hw, src_hw, ref_y0=0):
    """Source-map pixel index of every (view, item, plane, reference pixel): (ix, iy, qz), float64 [n_src,B,D,h,w].  ``ref_y0``: the
    h rows are rows [ref_y0, ref_y0 + h) of a larger reference grid whose cameras ``cams`` are."""
    assert geom in GEOMS
    h, w = int(ref_hw[0]), int(ref_hw[1])
    hs, ws = int(src_hw[0]), int(src_hw[1])
    cams = cams.detach().cpu().double()
    depth = depth.detach().cpu().double()
    n, B = cams.shape[:2]
    D = depth.shape[1]
    p = _pixels(geom, (h, w), ref_y0)                                                              # [3,hw]
    dv = depth.reshape(1, B, 1, D, -1)                                                             # [1,B,1,D,1|hw]
    m0 = cams[..., 0:9].reshape(n, B, 3, 3) @ p                                                    # [n,B,3,hw]
    if geom == "proj":
        q = m0.unsqueeze(3) * dv + cams[..., 9:12].reshape(n, B, 3, 1, 1)
    else:
        m1 = cams[..., 9:18].reshape(n, B, 3, 3) @ p
        q = m0.unsqueeze(3) - m1.unsqueeze(3) / (dv + 1e-9)
    q = q.expand(n, B, 3, D, h * w)
    qz = q[:, :, 2]
    front = qz > 0
    div = qz.clamp(min=1e-9) if geom == "homog" else torch.where(front, qz, torch.ones_like(qz))
    u = torch.where(front, q[:, :, 0] / div, torch.full_like(qz, -10.0))
    v = torch.where(front, q[:, :, 1] / div, torch.full_like(qz, -10.0))
    if geom == "proj":
        sx = sy = 1.0
        lo, hi = -4.5, 5.5
    else:
        sx, sy = (ws - 1) / ws, (hs - 1) / hs
        lo, hi = -0.05, 1.05
    ix = (u * sx).clamp(lo * (ws - 1), hi * (ws - 1))
    iy = (v * sy).clamp(lo * (hs - 1), hi * (hs - 1))
    shape = (n, B, D, h, w)
    return ix.reshape(shape), iy.reshape(shape), qz.reshape(shape)


def sample(src_cf, ix, iy):
    """src_cf [B,C,hs,ws] float64 sampled at pixel index (ix, iy) [B,D,h,w] -> [B,C,D,h,w]; zero padding."""
    B, C, hs, ws = src_cf.shape
    _, D, h, w = ix.shape
    grid = torch.stack((ix / ((ws - 1) / 2) - 1, iy / ((hs - 1) / 2) - 1), dim=-1).reshape(B, D * h, w, 2)
    return F.grid_sample(src_cf, grid, mode="bilinear", padding_mode="zeros", align_corners=True).reshape(B, C, D, h, w)


def cost_volume(ref_cf, warped, cost, temp=None):
    """The forward's output from the reference features [B,C,h,w] and the warped volumes [B,C,D,h,w]: [B,C,D,h,w] for the variance
    and soft-min statistics, [n,B,8,D,h,w] for the group-wise correlation, [n,B,C,D,h,w] for the plain warp."""
    assert cost in COSTS
    N = len(warped) + 1
    if cost == "warp_only":
        return torch.stack(list(warped))
    rv = ref_cf.unsqueeze(2)
    if cost in ("variance", "variance_cvp"):
        s, sq = rv, rv ** 2
        for wv in warped:
            s, sq = s + wv, sq + wv ** 2
        return sq / N - (s ** 2) / (N ** 2) if cost == "variance" else sq / N - (s / N) ** 2
    if cost == "softmin":
        sum_e, sum_v = 0.0, 0.0
        for wv in warped:
            diff = (rv - wv) ** 2
            e = torch.exp(-temp * diff.sum(dim=1, keepdim=True))
            sum_e, sum_v = sum_e + e, sum_v + e * diff
        return sum_v / (sum_e + 1e-6)
    out = []
    for wv in warped:                                 # 8 groups of C / 8 consecutive channels, summed products
        B, C = wv.shape[:2]
        out.append((rv.reshape(B, 8, C // 8, 1, *rv.shape[3:]) * wv.reshape(B, 8, C // 8, *wv.shape[2:])).sum(2))
    return torch.stack(out)


def _cf(x):          # channels-last [...,C] -> channels-first float64 (C behind the batch axis)
    x = x.detach().cpu().double()
    return x.movedim(-1, 1 if x.dim() in (4, 5) else 2).contiguous()


def backward(ref, srcs, cams, depth, grad_out, *, geom="proj", cost="variance", temp=0.0, ref_hw=None):
    """Gradients in float64 with the layouts of ``ops.warp_cost_bwd``: dict with ``dref`` [B,h,w,C] (None for the plain warp),
    ``dsrcs`` n x [B,hs,ws,C], ``dtemp`` [1] (soft-min, else None) with ``dtemp_cond`` = sum|per-voxel term| / |their sum| (how much
    of the temperature gradient cancels: a relative tolerance on it means that many times more on the terms), and for the bound
    tests ``gw`` n x [B,C,D,h,w] (the gradient with respect to each warped volume) and the sample positions ``ix`` / ``iy``
    [n,B,D,h,w].  Operands may have any floating type; their values are taken as they are."""
    srcs_cf = [_cf(s).requires_grad_(True) for s in srcs]
    B, C, hs, ws = srcs_cf[0].shape
    h, w = (ref.shape[1:3] if ref is not None else ((hs, ws) if ref_hw is None else ref_hw))
    ix, iy, _ = positions(cams, depth, geom, (h, w), (hs, ws))
    warped = [sample(s, ix[v], iy[v]) for v, s in enumerate(srcs_cf)]
    for wv in warped:
        wv.retain_grad()
    ref_cf = _cf(ref).requires_grad_(True) if cost != "warp_only" else None
    D = ix.shape[2]
    tt = torch.full((B, 1, D, h, w), float(temp), dtype=torch.float64, requires_grad=True)      # one copy per voxel: the terms of d temp
    vol = cost_volume(ref_cf, warped, cost, tt)
    g = _cf(grad_out)
    assert g.shape == vol.shape, (tuple(g.shape), tuple(vol.shape))
    vol.backward(g)
    cl = lambda x: x.permute(0, 2, 3, 1).contiguous()
    return {"dref": cl(ref_cf.grad) if ref_cf is not None else None,
            "dsrcs": [cl(s.grad) for s in srcs_cf],
            "dtemp": tt.grad.sum().reshape(1) if cost == "softmin" else None,
            "dtemp_cond": float(tt.grad.abs().sum() / tt.grad.sum().abs()) if cost == "softmin" else None,
            "gw": [wv.grad for wv in warped], "ix": ix, "iy": iy}


FWD_COSTS = COSTS + ("variance_partial",)


def variance_finish(sums, n_views, cost):
    """(sum f, sum f^2) [2,...] over ``n_views`` views -> the variance volume, with the two formulas of ``cost_volume``."""
    assert cost in ("variance", "variance_cvp")
    s, sq, N = sums[0].double(), sums[1].double(), int(n_views)
    return sq / N - (s ** 2) / (N ** 2) if cost == "variance" else sq / N - (s / N) ** 2


def forward(ref, srcs, cams, depth, *, geom, cost, temp=0.0, ref_hw=None, ref_y0=0):
    """The forward volume in float64 with the layout of ``ops.warp_cost``: [B,D,h,w,C] in general, [n,B,D,h,w,C/4] for the group
    correlation, [n,B,D,h,w,C] for the plain warp, [2,B,D,h,w,C] = (sum f, sum f^2) for ``variance_partial`` (over the reference and
    the warped views, or over the warped views alone when ``ref`` is None).  Returns (volume, ix, iy, qz), the last three
    [n,B,D,h,w].  ``ref`` / per-pixel ``depth`` are rows [ref_y0, ref_y0 + h) of the grid whose cameras ``cams`` are.  Operands may
    have any floating type; their values are taken as they are."""
    assert cost in FWD_COSTS
    srcs_cf = [_cf(s) for s in srcs]
    B, C, hs, ws = srcs_cf[0].shape
    h, w = (ref.shape[1:3] if ref is not None else ((hs, ws) if ref_hw is None else ref_hw))
    ix, iy, qz = positions(cams, depth, geom, (h, w), (hs, ws), ref_y0)
    warped = [sample(s, ix[v], iy[v]) for v, s in enumerate(srcs_cf)]
    ref_cf = _cf(ref) if (ref is not None and cost != "warp_only") else None
    if cost == "variance_partial":
        s = ref_cf.unsqueeze(2).expand_as(warped[0]).clone() if ref_cf is not None else torch.zeros_like(warped[0])
        sq = s ** 2
        for wv in warped:
            s, sq = s + wv, sq + wv ** 2
        vol = torch.stack((s, sq))
    else:
        vol = cost_volume(ref_cf, warped, cost, float(temp))
    return vol.movedim(1 if vol.dim() == 5 else 2, -1).contiguous(), ix, iy, qz


FRAGILE_EPS = 2.0 ** -18         # 32 fp32 ulps: sweep_index has six roundings and two rcp approximations of one ulp each
FRAGILE_TEXELS = 1.0 / 64


def fragile(cams, depth, geom, ref_hw, src_hw, ref_y0=0):
    """Boolean [n_src,B,D,h,w]: samples whose fp32 evaluation may legitimately land on the other side of the one discontinuity the
    warp has (q_z > 0 or not), or so far from the float64 position that a comparison of values says nothing.  From float64 alone.

    With e = 2^-18 and S(row) = sum of |terms| of a row of q (PROJ: the three products of ``rot p d`` and the addend ``trans``;
    HOMOG: the three terms of ``A p`` and the three of ``(Bm p) / (d + 1e-9)``), a sample is fragile when
    * |q_z| <= e S(z): the test ``hz > 0`` may flip.  EXACT ZEROS ARE EXEMPT: with S(z) == 0 every term of q_z is exactly zero, fp32
      computes exactly 0 as well and the sample is behind the camera on both sides -- a rig with such a sample checks ``>`` against ``>=``;
    * or, in front of the camera, the error of the index implied by the same relative bound on numerator and denominator,
      u +- e (S(x) + |u| S(z)) / q_z (and likewise for v), exceeds 1/64 texel: cancellation in hx, hy or hz.  The error is taken of the
      index that is sampled, i.e. after the index scale and the grid clamp: a position far beyond the clamp on both sides of its
      error interval has no error at all (next to q_z = 0 every u is huge, and clamped)."""
    assert geom in GEOMS
    h, w = int(ref_hw[0]), int(ref_hw[1])
    hs, ws = int(src_hw[0]), int(src_hw[1])
    cams = cams.detach().cpu().double()
    depth = depth.detach().cpu().double()
    n, B = cams.shape[:2]
    D = depth.shape[1]
    p = _pixels(geom, (h, w), ref_y0)
    dv = depth.reshape(1, B, 1, D, -1)
    M0 = cams[..., 0:9].reshape(n, B, 3, 3)
    a, sa = (M0 @ p).unsqueeze(3), (M0.abs() @ p.abs()).unsqueeze(3)                              # [n,B,3,1,hw]
    if geom == "proj":
        t = cams[..., 9:12].reshape(n, B, 3, 1, 1)
        q, S = a * dv + t, sa * dv.abs() + t.abs()
        sx = sy = 1.0
    else:
        M1 = cams[..., 9:18].reshape(n, B, 3, 3)
        dd = dv + 1e-9
        q, S = a - (M1 @ p).unsqueeze(3) / dd, sa + (M1.abs() @ p.abs()).unsqueeze(3) / dd.abs()
        sx, sy = (ws - 1) / ws, (hs - 1) / hs
    q, S = q.expand(n, B, 3, D, h * w), S.expand(n, B, 3, D, h * w)
    qz, Sz = q[:, :, 2], S[:, :, 2]
    sign = (qz.abs() <= FRAGILE_EPS * Sz) & (Sz > 0)
    front = qz > 0
    div = torch.where(front, qz, torch.ones_like(qz))
    lo, hi = (-4.5, 5.5) if geom == "proj" else (-0.05, 1.05)
    far = torch.zeros_like(front)
    for k, (scale, size) in enumerate(((sx, ws), (sy, hs))):
        u = q[:, :, k] / div
        du = FRAGILE_EPS * (S[:, :, k] + u.abs() * Sz) / div
        idx = lambda t: (t * scale).clamp(lo * (size - 1), hi * (size - 1))          # the index after the grid clamp: what is sampled
        far |= front & (torch.maximum(idx(u + du) - idx(u), idx(u) - idx(u - du)) > FRAGILE_TEXELS)
    return (sign | far).reshape(n, B, D, h, w)


def tap_scatter(ix, iy, gw, src_hw):
    """The bilinear scatter of one view written out by hand.  ix / iy [B,D,h,w], gw [B,C,D,h,w] -> per texel of the source map
    (taps [B,hs,ws] int64: number of (voxel, tap) pairs with a non-zero weight that land on it;
     abs_sum [B,hs,ws,C]: sum of |weight x gw| over them;  signed [B,hs,ws,C]: their sum, i.e. dsrc)."""
    hs, ws = int(src_hw[0]), int(src_hw[1])
    B, C = gw.shape[:2]
    x0, y0 = torch.floor(ix), torch.floor(iy)
    fx, fy = ix - x0, iy - y0
    x0, y0 = x0.long(), y0.long()
    g = gw.permute(0, 2, 3, 4, 1).reshape(-1, C)                                       # voxel-major like ix.reshape(-1)
    bidx = torch.arange(B).view(B, 1, 1, 1).expand_as(x0)
    taps = torch.zeros(B * hs * ws, dtype=torch.int64)
    abs_sum = torch.zeros(B * hs * ws, C, dtype=torch.float64)
    signed = torch.zeros(B * hs * ws, C, dtype=torch.float64)
    for dx, dy, wgt in ((0, 0, (1 - fx) * (1 - fy)), (1, 0, fx * (1 - fy)), (0, 1, (1 - fx) * fy), (1, 1, fx * fy)):
        tx, ty = x0 + dx, y0 + dy
        ok = (tx >= 0) & (tx < ws) & (ty >= 0) & (ty < hs) & (wgt != 0)
        flat = ((bidx * hs + ty.clamp(0, hs - 1)) * ws + tx.clamp(0, ws - 1)).reshape(-1)
        wv = torch.where(ok, wgt, torch.zeros_like(wgt)).reshape(-1, 1)
        taps.index_add_(0, flat, ok.reshape(-1).long())
        signed.index_add_(0, flat, g * wv)
        abs_sum.index_add_(0, flat, (g * wv).abs())
    return taps.reshape(B, hs, ws), abs_sum.reshape(B, hs, ws, C), signed.reshape(B, hs, ws, C)


# ---- the box rule of the tiled kernel, restated on the host (csrc/warp_bwd.hip, "exact bounding box ..." to the sub-pass choice) ----
TILE_W, TILE_H, TILE_PLANES = 16, 8, 4


def patch_texels(C):
    return 1024 if C <= 16 else 512


def _box(x0, y0, hs, ws, grow):
    """(bw, bh) of the texel box of the samples with integer corners x0 / y0 (1-D tensors), `grow` texels added to each extent."""
    ok = (x0 >= -1) & (x0 < ws) & (y0 >= -1) & (y0 < hs)
    if not bool(ok.any()):
        return 0, 0
    bx0, by0 = max(int(x0[ok].min()), 0), max(int(y0[ok].min()), 0)
    bx1, by1 = min(int(x0[ok].max()) + 1, ws - 1), min(int(y0[ok].max()) + 1, hs - 1)
    bw, bh = max(bx1 - bx0 + 1, 0), max(by1 - by0 + 1, 0)
    return (min(max(bw + grow, 0), ws), min(max(bh + grow, 0), hs)) if bw and bh else (bw, bh)


def box_regime(ix, iy, src_hw, C, tile=(0, 0), grow=0):
    """Regimes the tiled kernel takes for reference tile ``tile`` = (tile row, tile column) of ONE view and item (ix / iy [D,h,w]):
    the set over the depth chunks of "one" (the box fits the patch), "two" / "four" (row-group sub-passes whose boxes all fit) and
    "two_clipped" / "four_clipped" (a sub-pass box still beyond the capacity: clipped box plus direct atomics).  ``grow`` widens
    (or, negative, narrows) every box by that many texels each way: a test that names a regime asserts it for grow in (-1, 0, 1),
    so that a sample whose fp32 position falls on the other side of a texel edge than its float64 position cannot change it."""
    hs, ws = int(src_hw[0]), int(src_hw[1])
    cap = patch_texels(C)
    D, h, w = ix.shape
    ty, tx = tile
    ys, xs = slice(ty * TILE_H, min((ty + 1) * TILE_H, h)), slice(tx * TILE_W, min((tx + 1) * TILE_W, w))
    x0a, y0a = torch.floor(ix).long(), torch.floor(iy).long()
    seen = set()
    for d0 in range(0, D, TILE_PLANES):
        x0, y0 = x0a[d0:d0 + TILE_PLANES, ys, xs], y0a[d0:d0 + TILE_PLANES, ys, xs]
        bw, bh = _box(x0.reshape(-1), y0.reshape(-1), hs, ws, grow)
        nsub = 1 if bw * bh <= cap else (2 if bw * bh <= 2 * cap else 4)
        if nsub == 1:
            seen.add("one")
            continue
        rows = TILE_H // nsub
        clipped = False
        for sub in range(nsub):
            sx0, sy0 = x0[:, sub * rows:(sub + 1) * rows], y0[:, sub * rows:(sub + 1) * rows]
            if sx0.numel() == 0:
                continue
            sw, sh = _box(sx0.reshape(-1), sy0.reshape(-1), hs, ws, grow)
            clipped |= sw * sh > cap
        seen.add({2: "two", 4: "four"}[nsub] + ("_clipped" if clipped else ""))
    return seen


def fixed_point_quantum(grad_out, feats, n_src):
    """The quantum the tiled kernel documents for the variance statistic, from the launch-wide magnitude bound:
    q = 2^(floor(log2(Bmax)) - 20), Bmax = (2 / N) max|G| x 2 max|f|  (fp32 arithmetic in the kernel's order)."""
    inv_n = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(n_src + 1), dtype=torch.float32)
    gmax = (grad_out.detach().cpu().float() * 2.0 * inv_n).abs().max()
    fmax = max(float(f.detach().cpu().float().abs().max()) for f in feats)
    bmax = float(gmax * 2.0 * torch.tensor(fmax, dtype=torch.float32))
    return 2.0 ** (math.floor(math.log2(bmax)) - 20), bmax
