"""Float64 reference of the unsupervised training path: pscv_photo_warp(+_bwd), pscv_ssim(+_bwd) (csrc/photo_loss.hip) and the
function-level pscv_homography_warp(+_bwd) (csrc/homog_warp.hip), written from the rules of include/pscv.h with torch on the CPU.
It never imports ``wild_deep_mvs_amd.ops``.  tests/test_photo_ref_cpu.py pins it to the oracle evaluated in float64, to ATen's float64
grid_sample + autograd and to the goldens; tests/test_gpu_photo_ref.py holds the kernels to it element by element.

Error units.  Every result comes with a unit U built from ABSOLUTE values, like U of _conv2d_ref.py: a bound is ``ratio 2^-24 U``.
  * a matrix product carries  Uq_j = sum_k |proj_jk| (sum_l |inv_ref_kl| |p_l|);
  * scalar arithmetic behind it is propagated to first order by ``EV`` (value, unit): every operation adds the magnitude of its own
    result (one rounding) to what its operands carry, e.g. a / b -> (U_a + |a / b| U_b) / |b| + |a / b|;
  * a bilinear sample V(ix, iy) carries U_ix |dV/dix| + U_iy |dV/diy| + sum_k |w_k v_k|; within the position margin of an integer
    coordinate the larger one-sided slope counts (bilinear sampling is continuous: no sample is exempt);
  * a blur carries blur(|x|).
``fragile`` marks samples within ``POS_RATIO 2^-24 U`` of a decision (integer ix / iy, |g| = 1, |g| = 10, q_z = 0, q_z = 1e-6): an
fp32 evaluation may legitimately land on the other side.  The margin comes from the reference's unit, never from a kernel's output.

The rigs live in tests/_photo_rigs.py: literal matrices; each asserts, on this reference, that it reaches the regime it is named for."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from _warp_fwd_rigs import FRAGILE_CAP  # noqa: F401  (re-exported: the one cap of the warp families)

EPS = 2.0 ** -24
POS_RATIO = 8.0           # position bound in units of 2^-24 U_pos: the bound the z / flows outputs are held to (test_gpu_photo_ref.py)
ZMIN = float(np.float32(1e-6))          # clamp(min=1e-6) on an fp32 tensor compares with the fp32 value of 1e-6
HZMIN = float(np.float32(1e-9))
BEHIND, ZCL, XCL, YCL = 1, 2, 4, 8      # regime bits; 0 = free
D = torch.float64


class EV:
    """value + first-order error unit (in units of one fp32 rounding of an O(1) number)."""

    def __init__(self, v, e=None):
        self.v = v if torch.is_tensor(v) else torch.tensor(float(v), dtype=D)
        self.e = torch.zeros_like(self.v) if e is None else e

    @staticmethod
    def lift(x):
        return x if isinstance(x, EV) else EV(x)

    def __add__(self, o):
        o = EV.lift(o)
        v = self.v + o.v
        return EV(v, self.e + o.e + v.abs())
    __radd__ = __add__

    def __sub__(self, o):
        o = EV.lift(o)
        v = self.v - o.v
        return EV(v, self.e + o.e + v.abs())

    def __rsub__(self, o):
        return EV.lift(o) - self

    def __mul__(self, o):
        o = EV.lift(o)
        v = self.v * o.v
        return EV(v, self.e * o.v.abs() + o.e * self.v.abs() + v.abs())
    __rmul__ = __mul__

    def __truediv__(self, o):
        o = EV.lift(o)
        v = self.v / o.v
        return EV(v, (self.e + v.abs() * o.e) / o.v.abs() + v.abs())

    def __rtruediv__(self, o):
        return EV.lift(o) / self

    def __neg__(self):
        return EV(-self.v, self.e)


# =====================================================================================================================================
# photo warp
# =====================================================================================================================================
def _pix(h, w):
    ys, xs = torch.meshgrid(torch.arange(h, dtype=D), torch.arange(w, dtype=D), indexing="ij")
    return xs.reshape(-1), ys.reshape(-1)


def flows(depth, inv_ref, proj):
    """depth [B,h,w], inv_ref [B,4,4], proj [B,S,4,4] (any float type: the VALUES are what the kernel receives) -> dict of float64
    [B,S,h,w] maps: gx, gy (after the z <= 0 rule and the +-10 clamp), z = q_z, dgx, dgy = d g / d depth with the graph cut exactly
    where ATen cuts it (behind; the clamped axis, strictly outside +-10; d/dz in 0 < q_z <= 1e-6), regime bits, and the units
    Uz, Ugx, Ugy (of z and of g) and Udgx, Udgy.  NaN coordinates stay NaN (torch.clamp propagates them)."""
    depth, inv_ref, proj = depth.to(D), inv_ref.to(D), proj.to(D)
    B, h, w = depth.shape
    S = proj.shape[1]
    xs, ys = _pix(h, w)
    d = depth.reshape(B, -1)
    one = torch.ones_like(d)
    p = torch.stack((xs * d, ys * d, d, one), dim=-1)                             # [B,hw,4]
    dp = torch.stack((xs.expand_as(d), ys.expand_as(d), one, torch.zeros_like(d)), dim=-1)
    ai, ap = inv_ref.abs(), proj.abs()
    P3 = torch.einsum("bjk,bnk->bnj", inv_ref, p)
    q = torch.einsum("bsjk,bnk->bsnj", proj, P3)[..., :3]                         # [B,S,hw,3]
    Uq = torch.einsum("bsjk,bnk->bsnj", ap, torch.einsum("bjk,bnk->bnj", ai, p.abs()))[..., :3]
    dq = torch.einsum("bsjk,bnk->bsnj", proj, torch.einsum("bjk,bnk->bnj", inv_ref, dp))[..., :3]
    Udq = torch.einsum("bsjk,bnk->bsnj", ap, torch.einsum("bjk,bnk->bnj", ai, dp.abs()))[..., :3]
    qz = q[..., 2]
    behind = qz <= 0
    zcl = (qz > 0) & (qz <= ZMIN)
    zc = torch.where(torch.isnan(qz), qz, torch.clamp(qz, min=ZMIN))
    Z = EV(zc, torch.where(zcl | behind, torch.zeros_like(qz), Uq[..., 2]))
    out = {}
    regime = behind.long() * BEHIND + zcl.long() * ZCL
    for ax, size, bit in ((0, w, XCL), (1, h, YCL)):
        f = EV(q[..., ax], Uq[..., ax]) / Z
        g = 2.0 * f.v / (size - 1) - 1.0
        Ug = 2.0 * f.e / (size - 1) + g.abs() + 1.0
        # d f / d depth: (dq - f dq_z) / z in front, dq / 1e-6 where the clamp cuts d/dz
        dQ, dQz = EV(dq[..., ax], Udq[..., ax]), EV(dq[..., 2], Udq[..., 2])
        df_free = (dQ - f * dQz) / Z
        df_cut = dQ / Z
        df = torch.where(zcl, df_cut.v, df_free.v)
        Udf = torch.where(zcl, df_cut.e, df_free.e)
        g = torch.where(behind, torch.full_like(g, -10.0), g)
        cl = (g < -10.0) | (g > 10.0)                                             # ATen's clamp passes the gradient AT the bound
        gc = torch.where(torch.isnan(g), g, torch.clamp(g, -10.0, 10.0))
        cut = behind | cl
        dg = torch.where(cut, torch.zeros_like(g), 2.0 * df / (size - 1))
        dg = torch.where(torch.isnan(g), g, dg)
        Udg = torch.where(cut, torch.zeros_like(g), 2.0 * Udf / (size - 1) + dg.abs())
        Ug = torch.where(behind, torch.zeros_like(g), Ug)     # -10 exactly behind; a clamped value is continuous at the bound: keeps its unit
        regime = regime + (cl & ~behind).long() * bit
        k = "xy"[ax]
        # dg*_any: what the uncut expressions give (for the coarse bound of fragile samples), the larger of the two d/dz rules
        out.update({f"g{k}": gc.view(B, S, h, w), f"g{k}_raw": g.view(B, S, h, w), f"dg{k}": dg.view(B, S, h, w),
                    f"Ug{k}": Ug.view(B, S, h, w), f"Udg{k}": Udg.view(B, S, h, w),
                    f"dg{k}_any": (2.0 * torch.maximum(df_free.v.abs(), df_cut.v.abs()) / (size - 1)).view(B, S, h, w),
                    f"Ug{k}_raw": (2.0 * f.e / (size - 1) + g.abs() + 1.0).view(B, S, h, w)})
    out["z"], out["Uz"], out["regime"] = qz.view(B, S, h, w), Uq[..., 2].view(B, S, h, w), regime.view(B, S, h, w)
    return out


def index_of(g, Ug, size):
    """grid_sample(align_corners=False): ix = ((g + 1) size - 1) / 2 and its unit in texels."""
    ix = ((g + 1.0) * size - 1.0) * 0.5
    return ix, 0.5 * size * (Ug + (g + 1.0).abs()) + (g + 1.0).abs() * size * 0.5 + ix.abs()


def _bilinear(src, ix, iy):
    """src [N,C,hs,ws], ix / iy [N,h,w] in texels, zero padding -> V [N,C,h,w], dV/dix, dV/diy, cross = d2V/dix diy,
    A = sum_k |w_k v_k|, Ax / Ay = the absolute sums behind the two slopes.  NaN positions give NaN everywhere."""
    N, C, hs, ws = src.shape
    bad = torch.isnan(ix) | torch.isnan(iy)
    ixs, iys = torch.where(bad, torch.zeros_like(ix), ix), torch.where(bad, torch.zeros_like(iy), iy)
    x0, y0 = torch.floor(ixs), torch.floor(iys)
    ax, ay = (ixs - x0).unsqueeze(1), (iys - y0).unsqueeze(1)
    x0, y0 = x0.long(), y0.long()
    flat = src.reshape(N, C, -1)

    def tap(yy, xx):
        ok = (xx >= 0) & (xx < ws) & (yy >= 0) & (yy < hs)
        idx = (yy.clamp(0, hs - 1) * ws + xx.clamp(0, ws - 1)).reshape(N, 1, -1).expand(N, C, -1)
        v = torch.gather(flat, 2, idx).view(N, C, *ix.shape[1:])
        return torch.where(ok.unsqueeze(1), v, torch.zeros_like(v))
    v00, v01, v10, v11 = tap(y0, x0), tap(y0, x0 + 1), tap(y0 + 1, x0), tap(y0 + 1, x0 + 1)
    w00, w01, w10, w11 = (1 - ax) * (1 - ay), ax * (1 - ay), (1 - ax) * ay, ax * ay
    V = v00 * w00 + v01 * w01 + v10 * w10 + v11 * w11
    sx = (v01 - v00) * (1 - ay) + (v11 - v10) * ay
    sy = (v10 - v00) * (1 - ax) + (v11 - v01) * ax
    o = {"V": V, "sx": sx, "sy": sy, "cross": v11 - v10 - v01 + v00,
         "A": (v00 * w00).abs() + (v01 * w01).abs() + (v10 * w10).abs() + (v11 * w11).abs(),
         "Ax": (v01.abs() + v00.abs()) * (1 - ay) + (v11.abs() + v10.abs()) * ay,
         "Ay": (v10.abs() + v00.abs()) * (1 - ax) + (v11.abs() + v01.abs()) * ax}
    nan = torch.full_like(V, float("nan"))
    return {k: torch.where(bad.unsqueeze(1), nan, v) for k, v in o.items()}


def _sample(src, ix, iy, Uix, Uiy):
    """Value, slopes and the value's unit; the slopes in the unit are the larger of the one-sided ones within the position margin."""
    o = _bilinear(src, ix, iy)
    mx, my = (POS_RATIO * EPS * Uix), (POS_RATIO * EPS * Uiy)
    sxm, sym = o["sx"].abs(), o["sy"].abs()
    for dx, dy in ((-1, 0), (1, 0), (0, -1), (0, 1)):
        n = _bilinear(src, ix + dx * mx, iy + dy * my)
        sxm, sym = torch.maximum(sxm, n["sx"].abs()), torch.maximum(sym, n["sy"].abs())
    o["sx_max"], o["sy_max"] = sxm, sym
    o["U"] = Uix.unsqueeze(1) * sxm + Uiy.unsqueeze(1) * sym + o["A"]
    return o


def warp(src, gx, gy, Ugx=None, Ugy=None):
    """grid_sample(bilinear, zeros, align_corners=False) of src [N,C,hs,ws] at the normalised gx, gy [N,h,w]: a dict with V, the
    analytic dV/dix (``sx``) and dV/diy (``sy``) of the backward, the unit U, and mask = |g| < 1 strictly on all four sides."""
    src = src.to(D)
    hs, ws = src.shape[-2:]
    z = torch.zeros_like(gx)
    ix, Uix = index_of(gx, z if Ugx is None else Ugx, ws)
    iy, Uiy = index_of(gy, z if Ugy is None else Ugy, hs)
    o = _sample(src, ix, iy, Uix, Uiy)
    o.update({"ix": ix, "iy": iy, "Uix": Uix, "Uiy": Uiy,
              "mask": ((gx < 1) & (gy < 1) & (gx > -1) & (gy > -1)).to(D)})
    return o


def photo_warp(src, depth, inv_ref, proj, src_depth=None):
    """Everything pscv_photo_warp can write, with units: warped [B,S,C,h,w], mask, z, flows [B,S,h,w,2], warped_depth."""
    B, h, w = depth.shape
    S = proj.shape[1]
    fl = flows(depth, inv_ref, proj)
    gx, gy = fl["gx"].reshape(B * S, h, w), fl["gy"].reshape(B * S, h, w)
    Ugx, Ugy = fl["Ugx"].reshape(B * S, h, w), fl["Ugy"].reshape(B * S, h, w)
    r = {"fl": fl, "z": fl["z"], "Uz": fl["Uz"], "flows": torch.stack((fl["gx"], fl["gy"]), dim=-1),
         "Uflows": torch.stack((fl["Ugx"], fl["Ugy"]), dim=-1)}
    geo = warp(torch.zeros(B * S, 1, h, w, dtype=D), gx, gy, Ugx, Ugy)
    r["mask"] = geo["mask"].view(B, S, h, w)
    if src is not None and src.shape[2] > 0:
        C = src.shape[2]
        o = warp(src.reshape(B * S, C, h, w), gx, gy, Ugx, Ugy)
        r["warped"], r["Uwarped"], r["tap"] = o["V"].view(B, S, C, h, w), o["U"].view(B, S, C, h, w), o
    elif src is not None:
        r["warped"], r["Uwarped"] = torch.zeros(B, S, 0, h, w, dtype=D), torch.zeros(B, S, 0, h, w, dtype=D)
    if src_depth is not None:
        o = warp(src_depth.reshape(B * S, 1, h, w), gx, gy, Ugx, Ugy)
        r["warped_depth"], r["Uwarped_depth"] = o["V"].view(B, S, h, w), o["U"].view(B, S, h, w)
    return r


def warp_bwd(src, depth, inv_ref, proj, grad_warped, Ugw=None):
    """grad_depth [B,h,w] = sum_s ( sum_c gw dV/dix ) (w / 2) dgx + ( sum_c gw dV/diy ) (h / 2) dgy, its unit U, and ``coarse``: the
    sum of the magnitudes of the terms with the larger one-sided slope and EITHER derivative rule (what a fragile sample may give)."""
    B, S, C, h, w = src.shape
    gw = grad_warped.to(D).reshape(B * S, C, h, w)
    r = photo_warp(src, depth, inv_ref, proj)
    fl, o = r["fl"], r["tap"]
    v = lambda k: fl[k].reshape(B * S, h, w)
    gix, giy = (gw * o["sx"]).sum(1), (gw * o["sy"]).sum(1)
    dix, diy = 0.5 * w * v("dgx"), 0.5 * h * v("dgy")
    zero = torch.zeros_like(dix)
    tx = torch.where(dix == 0, zero, gix * dix)              # a cut gradient is a zero, whatever flows into it (ATen: where / masked)
    ty = torch.where(diy == 0, zero, giy * diy)
    nanpos = torch.isnan(v("gx")) | torch.isnan(v("gy"))
    term = torch.where(nanpos, torch.full_like(tx, float("nan")), tx + ty)
    g = term.view(B, S, h, w).sum(1)
    ag = gw.abs()
    Udix, Udiy = 0.5 * w * v("Udgx"), 0.5 * h * v("Udgy")
    U = ((ag * o["Ax"]).sum(1) + (ag * o["cross"].abs()).sum(1) * o["Uiy"]) * dix.abs() + gix.abs() * Udix \
        + ((ag * o["Ay"]).sum(1) + (ag * o["cross"].abs()).sum(1) * o["Uix"]) * diy.abs() + giy.abs() * Udiy + term.abs()
    if Ugw is not None:                                   # the unit the incoming gradient arrives with (end-to-end compositions)
        ug = Ugw.to(D).reshape(B * S, C, h, w)
        U = U + (ug * o["sx"].abs()).sum(1) * dix.abs() + (ug * o["sy"].abs()).sum(1) * diy.abs()
    U = U.view(B, S, h, w).sum(1) + g.abs()
    coarse = ((ag * o["sx_max"]).sum(1) * 0.5 * w * v("dgx_any") + (ag * o["sy_max"]).sum(1) * 0.5 * h * v("dgy_any"))
    coarse = 1.001 * coarse.view(B, S, h, w).sum(1) + g.abs() + 1e-30
    return {"grad": g, "U": U, "coarse": coarse}


def fragile(depth, inv_ref, proj, ratio=POS_RATIO):
    """[B,S,h,w] bool maps of the samples an fp32 evaluation may put on the other side of a decision:
    ``fwd``  q_z = 0 (the coordinate jumps to -10: every output but z);   ``mask``  fwd or |g| = 1;
    ``bwd``  fwd, q_z = 1e-6, |g| = 10, or an integer ix / iy (the bilinear derivative jumps)."""
    fl = flows(depth, inv_ref, proj)
    h, w = depth.shape[-2:]
    m = ratio * EPS
    near = lambda a, b, U: (a - b).abs() <= m * U
    fwd = near(fl["z"], 0.0, fl["Uz"])
    zmin = near(fl["z"], ZMIN, fl["Uz"])
    one = torch.zeros_like(fwd)
    ten, integer = one.clone(), one.clone()
    for k, size in (("x", w), ("y", h)):
        g, U = fl[f"g{k}_raw"], fl[f"Ug{k}_raw"]
        live = fl["z"] > 0
        one |= live & (near(g, 1.0, U) | near(g, -1.0, U))
        ten |= live & (near(g, 10.0, U) | near(g, -10.0, U))
        ix, Uix = index_of(fl[f"g{k}"], fl[f"Ug{k}"], size)
        integer |= (ix - torch.round(ix)).abs() <= m * Uix
    return {"fwd": fwd, "mask": fwd | one, "bwd": fwd | zmin | ten | integer}


# =====================================================================================================================================
# SSIM
# =====================================================================================================================================
def window():
    """make_window() of csrc/photo_loss.hip: exp in double, the normalisation an fp32 division -- its eleven fp32 values as float64."""
    v = np.array([math.exp(-((k - 5) ** 2) / (2.0 * 1.5 * 1.5)) for k in range(11)])
    s = np.float32(v.sum())
    return torch.from_numpy((v.astype(np.float32) / s).astype(np.float64))


def _blur(x):
    g = window()
    n, c = x.shape[:2]
    k = torch.outer(g, g).view(1, 1, 11, 11).expand(c, 1, 11, 11).contiguous()
    return F.conv2d(x, k, padding=5, groups=c)


C1, C2 = float(np.float32(0.01) * np.float32(0.01)), float(np.float32(0.03) * np.float32(0.03))


def _ssim_terms(img1, img2, rep, U2=None):
    """``U2``: the unit img2 itself arrives with (a warped image's), propagated to first order through the three blurs it enters."""
    a = img1.to(D).repeat_interleave(rep, dim=0)                                  # img1 item of img2 item n is n // rep
    b = img2.to(D)
    u = torch.zeros_like(b) if U2 is None else U2.to(D)
    mu1, mu2 = EV(_blur(a), _blur(a.abs())), EV(_blur(b), _blur(b.abs() + u))
    E11, E22 = EV(_blur(a * a), _blur(a * a)), EV(_blur(b * b), _blur(b * b + 2.0 * b.abs() * u))
    E12 = EV(_blur(a * b), _blur((a * b).abs() + a.abs() * u))
    s1, s2, s12 = E11 - mu1 * mu1, E22 - mu2 * mu2, E12 - mu1 * mu2
    A1, A2 = 2.0 * (mu1 * mu2) + C1, 2.0 * s12 + C2
    B1, B2 = mu1 * mu1 + mu2 * mu2 + C1, s1 + s2 + C2
    inv = 1.0 / (B1 * B2)
    S = A1 * A2 * inv
    return a, b, mu1, mu2, A1, A2, B1, B2, inv, S


def ssim(img1, img2, rep=1, U2=None):
    """1 - SSIM per channel and its unit.  img1 [n1,C,h,w], img2 [n1 rep,C,h,w], zero padding, the kernel's window."""
    S = _ssim_terms(img1, img2, rep, U2)[-1]
    out = 1.0 - S
    return {"out": out.v, "U": out.e}


def ssim_bwd(img1, img2, grad_out, rep=1, U2=None):
    """Gradient of sum(grad_out (1 - SSIM)) to img2: blur(a) + 2 img2 blur(b) + img1 blur(c) with (a, b, c) = -grad_out
    (dS/dmu2, dS/dE22, dS/dE12); the symmetric window's zero-padded blur is its own adjoint."""
    a, b, mu1, mu2, A1, A2, B1, B2, inv, S = _ssim_terms(img1, img2, rep, U2)
    dmu2 = 2.0 * mu1 * (A2 - A1) * inv - 2.0 * mu2 * S / B1 + 2.0 * mu2 * S / B2
    de22 = -(S / B2)
    de12 = 2.0 * A1 * inv
    go = -grad_out.to(D)
    ta, tb, tc = go * dmu2, go * de22, go * de12
    ba, bb, bc = _blur(ta.v), _blur(tb.v), _blur(tc.v)
    Ua, Ub, Uc = _blur(ta.e), _blur(tb.e), _blur(tc.e)                            # ta.e >= |ta|: covers the blur's own roundings
    g = ba + 2.0 * b * bb + a * bc
    U = Ua + 2.0 * b.abs() * Ub + a.abs() * Uc + ba.abs() + 2.0 * (2.0 * b * bb).abs() + 2.0 * (a * bc).abs() + g.abs()
    if U2 is not None:
        U = U + 2.0 * U2.to(D) * bb.abs()
    return {"grad": g, "U": U}


def photometricloss(imgs, depth, inv_ref, proj, up=(1.0, 1.0), mask=None):
    """Trainer.photometricloss + the masked mean + its backward, composed from the pieces above: ssim [B,S,h,w] (mean over the
    channels), mask, loss, grad_depth = d loss / d depth, with units that carry the upstream units along: ``up`` = (bound of
    ``warped`` / bound of ``ssim``, bound of ``ssim_bwd`` / bound of ``photo_warp_bwd``), so that one ratio bounds the chain.
    ``mask``: the mask to normalise with where it is not the reference's own -- a caller hands over the reference's mask with the
    kernel's decision at the ``fragile`` mask pixels (either value is legitimate there; everything downstream follows it exactly)."""
    B, N, C, h, w = imgs.shape
    S = N - 1
    src = imgs[:, 1:].to(D).contiguous()
    r = photo_warp(src, depth, inv_ref, proj)
    ref, wp, Uw = imgs[:, 0].to(D), r["warped"].reshape(B * S, C, h, w), r["Uwarped"].reshape(B * S, C, h, w) * up[0]
    s = ssim(ref, wp, S, U2=Uw)
    mask = r["mask"] if mask is None else mask.to(D)
    val, Uval = s["out"].view(B, S, C, h, w).mean(2), s["U"].view(B, S, C, h, w).mean(2)
    loss = (val * mask).sum() / mask.sum()
    go = (mask / mask.sum() / C).view(B * S, 1, h, w).expand(B * S, C, h, w)
    gb = ssim_bwd(ref, wp, go, S, U2=Uw)
    b = warp_bwd(src, depth, inv_ref, proj, gb["grad"].view(B, S, C, h, w), Ugw=gb["U"].view(B, S, C, h, w) * up[1])
    return {"ssim": val, "Ussim": Uval, "mask": mask, "loss": loss, "grad_depth": b["grad"], "Ugrad": b["U"], "coarse": b["coarse"],
            "warped": r["warped"]}


# =====================================================================================================================================
# function-level homography warp (channels-last image [m,hs,ws,c])
# =====================================================================================================================================
def homography_positions(H, ref_hw, src_hw):
    """H [m,3,3] or [m,h,w,3,3] -> ix, iy [m,h,w] in texels (align_corners=True after the +-1.1 clamp), their units, hz."""
    H = H.to(D)
    m = H.shape[0]
    h, w = ref_hw
    hs, ws = src_hw
    if H.dim() == 3:
        H = H.view(m, 1, 1, 3, 3).expand(m, h, w, 3, 3)
    xs, ys = _pix(h, w)
    p = torch.stack((xs + 0.5, ys + 0.5, torch.ones_like(xs)), dim=-1).view(1, h, w, 3)
    hom = torch.einsum("mhwjk,mhwk->mhwj", H, p.expand(m, h, w, 3))
    Uh = torch.einsum("mhwjk,mhwk->mhwj", H.abs(), p.expand(m, h, w, 3))
    hz = hom[..., 2]
    front = hz > 0
    zcl = front & (hz <= HZMIN)
    Z = EV(torch.clamp(hz, min=HZMIN), torch.where(zcl | ~front, torch.zeros_like(hz), Uh[..., 2]))
    res = []
    for ax, size in ((0, ws), (1, hs)):
        u = EV(hom[..., ax], Uh[..., ax]) / Z
        s = (size - 1) / size
        uv = torch.where(front, u.v, torch.full_like(u.v, -10.0))
        ue = torch.where(front, u.e, torch.zeros_like(u.e))
        raw = uv * s
        ix = torch.clamp(raw, -0.05 * (size - 1), 1.05 * (size - 1))
        clamped = ix != raw
        res += [ix, torch.where(clamped, ix.abs(), ue * s + 2.0 * raw.abs())]     # the fp32 clamp bound and (size-1)/size round once each
    return res[0], res[2], res[1], res[3], hz, Uh[..., 2]


def homography(img_cl, H, ref_hw):
    """img_cl [m,hs,ws,c] -> warped [m,h,w,c] and its unit."""
    img = img_cl.to(D).permute(0, 3, 1, 2)
    ix, iy, Uix, Uiy, _, _ = homography_positions(H, ref_hw, img.shape[-2:])
    o = _sample(img, ix, iy, Uix, Uiy)
    return {"out": o["V"].permute(0, 2, 3, 1), "U": o["U"].permute(0, 2, 3, 1), "ix": ix, "iy": iy}


def homography_bwd(grad_out_cl, H, src_hw):
    """Adjoint of ``homography`` to the image: grad_out [m,h,w,c] -> grad_image [m,hs,ws,c]; unit sum |g| (|w| + U_ix |dw/dix| +
    U_iy |dw/diy|) per texel (a tap's weight is continuous across an integer position: nothing is fragile)."""
    go = grad_out_cl.to(D)
    m, h, w, c = go.shape
    hs, ws = src_hw
    ix, iy, Uix, Uiy, _, _ = homography_positions(H, (h, w), src_hw)
    x0, y0 = torch.floor(ix), torch.floor(iy)
    fx, fy = ix - x0, iy - y0
    x0, y0 = x0.long(), y0.long()
    g = torch.zeros(m, hs * ws, c, dtype=D)
    U = torch.zeros(m, hs * ws, c, dtype=D)
    for dy, dx, wgt, dwx, dwy in ((0, 0, (1 - fx) * (1 - fy), 1 - fy, 1 - fx), (0, 1, fx * (1 - fy), 1 - fy, fx),
                                  (1, 0, (1 - fx) * fy, fy, 1 - fx), (1, 1, fx * fy, fy, fx)):
        xx, yy = x0 + dx, y0 + dy
        ok = ((xx >= 0) & (xx < ws) & (yy >= 0) & (yy < hs)).to(D)
        idx = (yy.clamp(0, hs - 1) * ws + xx.clamp(0, ws - 1)).view(m, -1, 1).expand(m, h * w, c)
        wv = (wgt * ok).view(m, -1, 1)
        wu = ((wgt + Uix * dwx + Uiy * dwy) * ok).view(m, -1, 1)
        g.scatter_add_(1, idx, go.reshape(m, -1, c) * wv)
        U.scatter_add_(1, idx, go.reshape(m, -1, c).abs() * wu)
    return {"grad": g.view(m, hs, ws, c), "U": U.view(m, hs, ws, c)}
