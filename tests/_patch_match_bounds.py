"""Error model of csrc/patch_match.hip beside the float64 rule of tests/_patch_match_ref.py.

Every fp32 step of the kernel is restated in float64 as a value with an absolute error bound (class ``E``): a running error
analysis.  An operation z = x op y carries the propagated error of its operands (second-order term included) plus one unit
``U = 2^-24`` times the magnitude of the result per rounding of that step; a step whose operands are exact and whose float64
result is an fp32 number is exact (hand-built dyadic cases rely on it).  The float64 window sums add no counted rounding.  The
constants that are not one-per-operation are named below, each next to the count it comes from.  From these:

  cost_model       per (source, pixel): c_ref, a bound on |c_kernel - c_ref|, and each validity criterion as (truth, decided)
  geom_model       per (source, pixel): e_s, its bound, whether its decisions (the rounding of the forward projection first) are
                   decided, and where the kernel must return e_max exactly
  aggregate_model  the top_k mean and its bound (a mean of order statistics is 1-Lipschitz in the largest per-source error)
  filter_model     per (source, pixel): passes / decided, for the three filter tests
  candidate_model  the 11 candidates, per-element bounds, the ``live`` decisions

and the checks that the CPU emulation (tests/_patch_match_emu.py) and the GPU kernel both go through (``check_*``): they count
violations and report the worst |got - ref| / bound; nothing exempts a pixel as a whole.
"""
from __future__ import annotations

import math

import numpy as np

from tests import _patch_match_ref as PR
from tests._fusion_ref import cam_rows

F = np.float64
U = 2.0 ** -24

# __expf(x) is exp2(x * log2(e)) on the hardware exponential: the product's rounding and the fp32 log2(e) move the result by
# 1.5 |x| U relative (counted 2 |x|), the hardware exp2 is good to one ulp = 2 U (counted 4)
K_EXP_ARG, K_EXP_HW = 2.0, 4.0
# pm_bilinear: u - x0, 1 - fx, two products and a sum per row (4 on the longest path), 1 - fy, a product and the last sum: 8
# roundings of at most the largest of the four texels
K_INTERP = 8.0
# __sinf / __cosf of an angle in [0, 2 pi): the angle's product, the product with the fp32 1 / (2 pi) and that constant are
# 2.5 roundings of up to 2 pi = 16 U absolute; the ISA gives no figure for the hardware sine itself, it is allowed 112 U more
K_SINCOS = 128.0
# the float64 sums are not counted; this covers their own rounding and the float64 evaluation of the model itself
SLOP64 = 1e-12

# Tightening: the analytic bounds are worst-case sums (every rounding of the homography chain pushing the same way); a check whose
# worst measured |kernel - float64 reference| / bound on the MI355X is below 0.25 over all cases is too loose to catch a subtle
# error, and its bar is 4 x that worst ratio.  1.0 = the analytic bound stands (worst measured: candidates 0.83, init 0.50,
# e_s 0.287 in the exact rm-edge case, whose short chain leaves the bound little slack).
# Worst measured against the analytic bound: cost 0.0234, aggregate 0.179, regret 4.03e-4.
SCALE = dict(cost=4 * 0.0234, err=1.0, agg=4 * 0.179, regret=4 * 4.03e-4, cand=1.0, init=1.0)

MIN_VAR32 = float(np.float32(PR.MIN_VAR))
COS1_32 = float(np.float32(0.99984769515639123916))
COS3_32 = float(np.float32(0.99862953475457387378))
LAMBDA32 = float(np.float32(PR.GEOM_LAMBDA))
MAXCOST32 = float(np.float32(PR.FILTER_MAX_COST))


def _rep32(z):
    with np.errstate(all="ignore"):
        return z.astype(np.float32).astype(F) == z


class E:
    """float64 value ``v`` of an fp32 quantity of the kernel with a bound ``e`` on |kernel - v|."""
    __slots__ = ("v", "e")

    def __init__(self, v, e=None):
        self.v = np.asarray(v, dtype=F)
        self.e = np.zeros(self.v.shape) if e is None else np.broadcast_to(np.asarray(e, dtype=F), self.v.shape)

    @property
    def shape(self):
        return self.v.shape

    def __getitem__(self, k):
        return E(self.v[k], self.e[k])

    def sum(self, axis):
        return E(self.v.sum(axis), self.e.sum(axis))

    def __add__(self, o): return add(self, o)
    def __radd__(self, o): return add(o, self)
    def __sub__(self, o): return sub(self, o)
    def __rsub__(self, o): return sub(o, self)
    def __mul__(self, o): return mul(self, o)
    def __rmul__(self, o): return mul(o, self)
    def __truediv__(self, o): return div(self, o)
    def __rtruediv__(self, o): return div(o, self)
    def __neg__(self): return E(-self.v, self.e)


def _c(x):
    return x if isinstance(x, E) else E(x)


def const(rule, kernel):
    """A constant of the rule whose fp32 value in the kernel is ``kernel``."""
    return E(rule, abs(float(kernel) - float(rule)))


def _mk(z, ep, r, exact_in):
    with np.errstate(all="ignore"):
        e = ep
        if r:
            e = ep + np.where(exact_in & _rep32(z), 0.0, r * U * (np.abs(z) + ep))
        e = np.where(np.isnan(e) & ~np.isnan(z), np.inf, e)
        e = np.where(np.abs(z) > 1e37, np.inf, e)              # fp32 overflows where float64 does not
    return E(z, e)


def add(x, y, r=1):
    x, y = _c(x), _c(y)
    with np.errstate(all="ignore"):
        return _mk(x.v + y.v, x.e + y.e, r, (x.e == 0) & (y.e == 0))


def sub(x, y, r=1):
    x, y = _c(x), _c(y)
    with np.errstate(all="ignore"):
        return _mk(x.v - y.v, x.e + y.e, r, (x.e == 0) & (y.e == 0))


def mul(x, y, r=1):
    x, y = _c(x), _c(y)
    with np.errstate(all="ignore"):
        ep = np.abs(x.v) * y.e + np.abs(y.v) * x.e + x.e * y.e
        ep = np.where((x.e == 0) & (y.e == 0), 0.0, ep)        # 0 * inf of an exact operand is not an error
        return _mk(x.v * y.v, ep, r, (x.e == 0) & (y.e == 0))


def div(x, y, r=1):
    x, y = _c(x), _c(y)
    with np.errstate(all="ignore"):
        z = x.v / y.v
        room = np.abs(y.v) - y.e
        ep = np.where(room > 0, (x.e + np.abs(z) * y.e) / np.where(room > 0, room, 1.0), np.inf)
        ep = np.where((x.e == 0) & (y.e == 0), 0.0, ep)
        return _mk(z, ep, r, (x.e == 0) & (y.e == 0))


def sqrt(x, r=1):
    x = _c(x)
    with np.errstate(all="ignore"):
        z = np.sqrt(np.maximum(x.v, 0.0))
        z = np.where(np.isnan(x.v), np.nan, z)
        ep = np.minimum(np.where(z > 0, x.e / np.where(z > 0, z, 1.0), np.inf), np.sqrt(x.e))
        return _mk(z, ep, r, x.e == 0)


def clamp(x, lo, hi):
    """fminf(fmaxf(x, lo), hi): 1-Lipschitz, NaN -> lo."""
    return E(np.clip(np.where(np.isnan(x.v), lo, x.v), lo, hi), np.where(np.isnan(x.v), 0.0, x.e))


def xadd(x, y): return add(x, y, 0)
def xsub(x, y): return sub(x, y, 0)
def xmul(x, y): return mul(x, y, 0)
def xdiv(x, y): return div(x, y, 0)
def xsqrt(x): return sqrt(x, 0)


def esincos(x):
    """(__sinf, __cosf) of an angle."""
    e = x.e + K_SINCOS * U
    return E(np.sin(x.v), e), E(np.cos(x.v), e)


# ---------------------------------------------------------------------------------------------------------------------------
# decisions: (truth of the float64 value, decided = the whole interval agrees).  NaN compares false on both sides: decided.
# ---------------------------------------------------------------------------------------------------------------------------
def _dec(x, thr, op, slack=0.0):
    x = _c(x)
    with np.errstate(all="ignore"):
        e = np.where(x.e + slack == 0, 0.0, x.e + slack + SLOP64 * (1.0 + np.abs(x.v)))     # an exact value decides itself
        lo, hi = op(x.v - e, thr), op(x.v + e, thr)
        t = op(x.v, thr)
        dec = (lo == hi) & (lo == t) | np.isnan(x.v)
        dec &= ~(np.isinf(e) & ~np.isnan(x.v))
    return t, dec


def gt(x, thr, slack=0.0): return _dec(x, thr, np.greater, slack)
def ge(x, thr, slack=0.0): return _dec(x, thr, np.greater_equal, slack)
def le(x, thr, slack=0.0): return _dec(x, thr, np.less_equal, slack)
def lt(x, thr, slack=0.0): return _dec(x, thr, np.less, slack)


def combine(parts):
    """All parts true; decided when every part is, or a decided part is false."""
    t = np.logical_and.reduce([p[0] for p in parts])
    alldec = np.logical_and.reduce([p[1] for p in parts])
    anyfalse = np.logical_or.reduce([p[1] & ~p[0] for p in parts])
    return t, alldec | anyfalse


# ---------------------------------------------------------------------------------------------------------------------------
# geometry blocks (pm_source_block), in the kernel's association
# ---------------------------------------------------------------------------------------------------------------------------
def _dot3(a0, b0, a1, b1, a2, b2):
    return a0 * b0 + a1 * b1 + a2 * b2


def _mat3mul(a, b):
    return [_dot3(a[3 * i], b[j], a[3 * i + 1], b[3 + j], a[3 * i + 2], b[6 + j]) for i in range(3) for j in range(3)]


def source_blocks(cams, wrap=E):
    """27 arrays [S]: A (0-8), b (9-11), C (12-14), G (15-23), c (24-26), as pm_source_block rounds them (``wrap`` = E for the
    model, an fp32 array for the emulation: the association is the same)."""
    c = cam_rows(cams)
    S = c.shape[0] - 1
    r = [wrap(np.full(S, c[0, k])) for k in range(30)]
    s = [wrap(c[1:, k]) for k in range(30)]
    rK, rKi, rR, rt = r[0:9], r[9:18], r[18:27], r[27:30]
    cK, cKi, cR, ct = s[0:9], s[9:18], s[18:27], s[27:30]
    Rr = [_dot3(cR[3 * i], rR[3 * j], cR[3 * i + 1], rR[3 * j + 1], cR[3 * i + 2], rR[3 * j + 2]) for i in range(3) for j in range(3)]
    tr = [ct[i] - _dot3(Rr[3 * i], rt[0], Rr[3 * i + 1], rt[1], Rr[3 * i + 2], rt[2]) for i in range(3)]
    C = [-_dot3(Rr[i], tr[0], Rr[3 + i], tr[1], Rr[6 + i], tr[2]) for i in range(3)]
    RrT = [Rr[3 * j + i] for i in range(3) for j in range(3)]
    A = _mat3mul(_mat3mul(cK, Rr), rKi)
    b = [_dot3(cK[3 * i], tr[0], cK[3 * i + 1], tr[1], cK[3 * i + 2], tr[2]) for i in range(3)]
    G = _mat3mul(_mat3mul(rK, RrT), cKi)
    cc = [_dot3(rK[3 * i], C[0], rK[3 * i + 1], C[1], rK[3 * i + 2], C[2]) for i in range(3)]
    return A + b + C + G + cc


def _kinv(cams):
    c = cam_rows(cams)
    return [E(c[0, 9 + i]) for i in range(9)]


def _f32(x):
    return np.asarray(x, dtype=np.float32).astype(F)


# ---------------------------------------------------------------------------------------------------------------------------
# samples
# ---------------------------------------------------------------------------------------------------------------------------
class _Image:
    """A grey image with the one-sided slopes of its clamped bilinear interpolant: LX[y0, x0] bounds |dI/du| over the cell
    (x0, y0) and its eight neighbours (what an error box of under one texel can touch), LY the same for v; CX, CY over the cell
    alone."""

    def __init__(self, img):
        self.I = np.asarray(img, dtype=np.float32).astype(F)
        h, w = self.I.shape
        hd, vd = np.zeros((h, w)), np.zeros((h, w))
        hd[:, : w - 1] = np.abs(np.diff(self.I, axis=1))
        vd[: h - 1] = np.abs(np.diff(self.I, axis=0))

        def nmax(a, ry, rx):
            p = np.pad(a, 2)
            out = np.zeros((h, w))
            for dy in ry:
                for dx in rx:
                    out = np.maximum(out, p[2 + dy: 2 + dy + h, 2 + dx: 2 + dx + w])
            return out
        self.LX = nmax(hd, (-1, 0, 1, 2), (-1, 0, 1))
        self.LY = nmax(vd, (-1, 0, 1), (-1, 0, 1, 2))
        self.CX = nmax(hd, (0, 1), (0,))                       # the cell alone: rows y0, y0 + 1 / columns x0, x0 + 1
        self.CY = nmax(vd, (0,), (0, 1))
        self.range = float(self.I.max() - self.I.min())
        self.amax = float(np.abs(self.I).max())

    def sample(self, u, v):
        """E of pm_bilinear at the E position (u, v)."""
        h, w = self.I.shape
        with np.errstate(all="ignore"):
            val = PR._bilinear(self.I, u.v, v.v)
            uc = np.clip(np.nan_to_num(u.v, nan=0.0), 0.0, w - 1.0)
            vc = np.clip(np.nan_to_num(v.v, nan=0.0), 0.0, h - 1.0)
            x0, y0 = np.floor(uc).astype(np.int64), np.floor(vc).astype(np.int64)
            eu = np.where(np.isnan(u.v) | np.isnan(u.e), np.inf, u.e)
            ev = np.where(np.isnan(v.v) | np.isnan(v.e), np.inf, v.e)
            # an error box that stays inside the texel cell (and inside the image) sees the cell's own slopes only
            own = (uc - x0 > eu) & (x0 + 1 - uc > eu) & (vc - y0 > ev) & (y0 + 1 - vc > ev) & (uc == u.v) & (vc == v.v)
            lx, ly = np.where(own, self.CX[y0, x0], self.LX[y0, x0]), np.where(own, self.CY[y0, x0], self.LY[y0, x0])
            e = np.where(lx > 0, lx * eu, 0.0) + np.where(ly > 0, ly * ev, 0.0)
            e = np.where((eu < 1.0) & (ev < 1.0) & np.isfinite(e), e, np.inf)
            e = np.minimum(e, self.range) + K_INTERP * U * self.amax
        return E(val, e)


# ---------------------------------------------------------------------------------------------------------------------------
# the reference window (the kernel's prologue)
# ---------------------------------------------------------------------------------------------------------------------------
def window_model(ref, rows, cols, radius, step):
    h, w = ref.shape
    oy, ox = PR.offsets(radius, step)
    R = np.asarray(ref, dtype=np.float32).astype(F)
    rr = np.clip(rows[:, None] + oy[None], 0, h - 1)
    cc = np.clip(cols[:, None] + ox[None], 0, w - 1)
    rp = E(R[rr, cc]) - E(R[rows, cols][:, None])
    f = np.float32
    inv2ss = const(1.0 / (2.0 * radius * radius), f(1.0) / (f(2.0) * f(radius) * f(radius)))
    inv2sc = const(1.0 / (2.0 * PR.SIGMA_COLOR ** 2), f(1.0) / (f(2.0) * f(PR.SIGMA_COLOR) * f(PR.SIGMA_COLOR)))
    arg = E(-(oy ** 2 + ox ** 2)[None].astype(F)) * inv2ss - (rp * rp) * inv2sc
    wv = np.exp(arg.v)
    wgt = E(wv, wv * (np.expm1(arg.e) + (K_EXP_ARG * np.abs(arg.v) + K_EXP_HW) * U))
    wr = wgt * rp
    W = wgt.sum(1)
    inv_w = xdiv(1.0, W)
    mr = xmul(wr.sum(1), inv_w)
    vr = xsub(xmul(xmul(wr, rp).sum(1), inv_w), xmul(mr, mr))
    return dict(wgt=wgt, wr=wr, rp=rp, inv_w=inv_w, mr=mr, vr=vr, oy=oy, ox=ox)


# ---------------------------------------------------------------------------------------------------------------------------
# photometric cost
# ---------------------------------------------------------------------------------------------------------------------------
CRITERIA = ("front", "u_lo", "u_hi", "v_lo", "v_hi", "var_r", "var_s", "angle")


def cost_model(ref, srcs, cams, rows, cols, depth, normal, radius=5, step=1, window=None):
    """-> dict: c [S,N] the rule's cost, cb [S,N] the bound on |c_kernel - c| where the source is valid on both sides, valid /
    vdec [S,N], crit {name: (truth, decided)} [S,N], cos E [S,N] (the angle's cosine), craw E [S,N] (the cost before validity)."""
    S, N = len(srcs), len(rows)
    G = source_blocks(cams)
    kinv = _kinv(cams)
    win = window_model(ref, rows, cols, radius, step) if window is None else window
    col, row = E(cols.astype(F)), E(rows.astype(F))
    d = E(_f32(depth))
    n = [E(_f32(np.asarray(normal)[:, i])) for i in range(3)]
    m = [kinv[3 * i] * col + kinv[3 * i + 1] * row + kinv[3 * i + 2] for i in range(3)]
    rho = d * (n[0] * m[0] + n[1] * m[1] + n[2] * m[2])
    ir = 1.0 / rho
    g = [(kinv[i] * n[0] + kinv[3 + i] * n[1] + kinv[6 + i] * n[2]) * ir for i in range(3)]
    X = [d * m[i] for i in range(3)]
    nX = sqrt(X[0] * X[0] + X[1] * X[1] + X[2] * X[2])
    qx, qy = E((cols[:, None] + win["ox"][None]).astype(F)), E((rows[:, None] + win["oy"][None]).astype(F))
    vr_dec = ge(win["vr"], PR.MIN_VAR, abs(MIN_VAR32 - PR.MIN_VAR))
    out = dict(c=np.full((S, N), 2.0), cb=np.zeros((S, N)), valid=np.zeros((S, N), bool), vdec=np.zeros((S, N), bool),
               crit={k: (np.zeros((S, N), bool), np.zeros((S, N), bool)) for k in CRITERIA},
               cos=E(np.zeros((S, N)), np.zeros((S, N))), craw=E(np.zeros((S, N)), np.zeros((S, N))), window=win)
    cosv, cose, rawv, rawe = np.zeros((S, N)), np.zeros((S, N)), np.zeros((S, N)), np.zeros((S, N))
    for s in range(S):
        img = _Image(srcs[s])
        hs, ws = img.I.shape
        gs = [x[s] for x in G]
        H = [gs[3 * i + j] + gs[9 + i] * g[j] for i in range(3) for j in range(3)]
        xc = [H[3 * i] * col + H[3 * i + 1] * row + H[3 * i + 2] for i in range(3)]
        uc, vc = xc[0] / xc[2], xc[1] / xc[2]
        r = [X[i] - gs[12 + i] for i in range(3)]
        cosa = (X[0] * r[0] + X[1] * r[1] + X[2] * r[2]) / (nX * sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]))
        Ht = [x[:, None] for x in H]
        x = [Ht[3 * i] * qx + Ht[3 * i + 1] * qy + Ht[3 * i + 2] for i in range(3)]
        iz = 1.0 / x[2]
        u, v = x[0] * iz, x[1] * iz
        pt, pd = gt(x[2], 0.0)
        u = E(np.where(pt, u.v, 0.0), np.where(pd, np.where(pt, u.e, 0.0), np.inf))      # a tap behind reads (0, 0)
        v = E(np.where(pt, v.v, 0.0), np.where(pd, np.where(pt, v.e, 0.0), np.inf))
        val = img.sample(u, v)
        val = E(val.v, np.where(pd & ~pt, 0.0, val.e))
        sc = img.sample(uc, vc)
        sp = val - sc[:, None]
        wv = xmul(win["wgt"], sp)
        ms = xmul(wv.sum(1), win["inv_w"])
        vs = xsub(xmul(xmul(wv, sp).sum(1), win["inv_w"]), xmul(ms, ms))
        cov = xsub(xmul(xmul(win["wr"], sp).sum(1), win["inv_w"]), xmul(win["mr"], ms))
        ncc = xdiv(cov, xsqrt(xmul(win["vr"], vs)))
        craw = clamp(1.0 - add(ncc, 0.0), 0.0, 2.0)            # the cast to fp32 and the subtraction: two roundings
        parts = dict(front=gt(xc[2], 0.0), u_lo=ge(uc, 0.0), u_hi=le(uc, ws - 1.0), v_lo=ge(vc, 0.0), v_hi=le(vc, hs - 1.0),
                     var_r=vr_dec, var_s=ge(vs, PR.MIN_VAR, abs(MIN_VAR32 - PR.MIN_VAR)),
                     angle=le(cosa, math.cos(math.radians(PR.MIN_TRI_DEG)), abs(COS1_32 - math.cos(math.radians(PR.MIN_TRI_DEG)))))
        valid, vdec = combine(list(parts.values()))
        # a criterion behind a decidedly false one is never evaluated: it counts as decided
        dead = np.logical_or.reduce([p[1] & ~p[0] for p in parts.values()])
        for k in CRITERIA:
            out["crit"][k][0][s], out["crit"][k][1][s] = parts[k][0], parts[k][1] | dead
        out["valid"][s], out["vdec"][s] = valid, vdec
        out["c"][s] = np.where(valid, craw.v, 2.0)
        with np.errstate(all="ignore"):
            out["cb"][s] = np.minimum(np.where(np.isfinite(craw.e), craw.e, 2.0) + SLOP64, 2.0)
        cosv[s], cose[s], rawv[s], rawe[s] = cosa.v, cosa.e, craw.v, out["cb"][s]
    out["cos"], out["craw"] = E(cosv, cose), E(rawv, rawe)
    return out


def undecided_share(cm):
    """Share of the (source, pixel, criterion) triples whose decision is undecided."""
    und = sum(int((~cm["crit"][k][1]).sum()) for k in CRITERIA)
    return und / (len(CRITERIA) * cm["valid"].size)


# ---------------------------------------------------------------------------------------------------------------------------
# forward-backward error
# ---------------------------------------------------------------------------------------------------------------------------
def geom_model(cams, src_depths, rows, cols, depth):
    """-> dict: e [S,N] the rule's e_s, eb [S,N] its bound, dec [S,N] every decision decided, rdec [S,N] the two roundings decided
    (true where an earlier decision already returned e_max), exact3 [S,N] decidedly e_max (invalid or capped)."""
    S, N = len(src_depths), len(rows)
    G = source_blocks(cams)
    col, row = E(cols.astype(F)), E(rows.astype(F))
    d = E(_f32(depth))
    out = dict(e=np.full((S, N), PR.GEOM_EMAX), eb=np.zeros((S, N)), dec=np.zeros((S, N), bool), rdec=np.zeros((S, N), bool),
               exact3=np.zeros((S, N), bool))
    for s in range(S):
        g = [x[s] for x in G]
        Ds = np.asarray(src_depths[s], dtype=np.float32).astype(F)
        hs, ws = Ds.shape
        y = [d * (g[3 * i] * col + g[3 * i + 1] * row + g[3 * i + 2]) + g[9 + i] for i in range(3)]
        front = gt(y[2], 0.0)
        u, v = y[0] / y[2], y[1] / y[2]
        with np.errstate(all="ignore"):
            big = combine([lt(E(np.abs(u.v), u.e), 2.0 ** 30), lt(E(np.abs(v.v), v.e), 2.0 ** 30)])
            fin = front[0] & big[0]
            uu, vv = np.where(fin, u.v, 0.0), np.where(fin, v.v, 0.0)
            au, av = np.abs(uu), np.abs(vv)
            ue, ve = np.where(fin, u.e, 0.0), np.where(fin, v.e, 0.0)
            # decided: the half-integer is further than the position error, or the position is exact (then so is the kernel's)
            rdec = ((np.abs(au - np.floor(au) - 0.5) > ue + SLOP64 * (1 + au)) | (ue == 0)) \
                & ((np.abs(av - np.floor(av) - 0.5) > ve + SLOP64 * (1 + av)) | (ve == 0))
        qx = (np.sign(uu) * np.floor(au + 0.5)).astype(np.int64)
        qy = (np.sign(vv) * np.floor(av + 0.5)).astype(np.int64)
        ins = (qx >= 0) & (qx < ws) & (qy >= 0) & (qy < hs)
        ds = np.where(ins, Ds[np.clip(qy, 0, hs - 1), np.clip(qx, 0, ws - 1)], 0.0)
        dpos = ds > 0                                          # NaN depth: false on both sides
        fx, fy, dse = E(qx.astype(F)), E(qy.astype(F)), E(np.where(dpos, ds, 1.0))
        r = [dse * (g[15 + 3 * i] * fx + g[16 + 3 * i] * fy + g[17 + 3 * i]) + g[24 + i] for i in range(3)]
        rpos = gt(r[2], 0.0)
        ex, ey = r[0] / r[2] - col, r[1] / r[2] - row
        err = sqrt(ex * ex + ey * ey)
        round_part = (np.ones(N, bool), rdec)
        valid, dec = combine([front, big, round_part, (ins, rdec), (dpos, rdec), (rpos[0], rpos[1] & rdec)])
        early = (front[1] & ~front[0]) | (big[1] & ~big[0])
        capped = gt(err, PR.GEOM_EMAX)
        with np.errstate(all="ignore"):
            out["e"][s] = np.where(valid, np.minimum(err.v, PR.GEOM_EMAX), PR.GEOM_EMAX)
            out["eb"][s] = np.where(valid, np.where(np.isfinite(err.e), err.e, PR.GEOM_EMAX) + SLOP64, 0.0)
        out["dec"][s] = dec
        out["rdec"][s] = rdec | early
        out["exact3"][s] = dec & (~valid | (capped[0] & capped[1]))
    return out


def aggregate_model(cm, gm, top_k):
    """The aggregated cost [N] and the bound on |agg_kernel - agg|: the largest per-source error (an undecided validity can move
    a source between its cost and 2, an undecided e_s anywhere in [0, e_max]) plus the top_k sums and the division."""
    val = cm["c"].copy()
    with np.errstate(all="ignore"):
        b = np.where(cm["vdec"], np.where(cm["valid"], cm["cb"], 0.0), np.abs(2.0 - cm["craw"].v) + cm["cb"])
        if gm is not None:
            val = val + PR.GEOM_LAMBDA * np.minimum(gm["e"], PR.GEOM_EMAX)
            be = np.where(gm["dec"], np.where(gm["exact3"], 0.0, gm["eb"]), PR.GEOM_EMAX)
            b = b + LAMBDA32 * be + abs(LAMBDA32 - PR.GEOM_LAMBDA) * PR.GEOM_EMAX + 2 * U * np.abs(val)   # product and sum
    agg = PR.aggregate(val, top_k)
    return agg, b.max(0) + (top_k + 1) * U * np.abs(val).max(0) + SLOP64, val


# ---------------------------------------------------------------------------------------------------------------------------
# filter
# ---------------------------------------------------------------------------------------------------------------------------
FILTER_CRITERIA = ("cost", "angle3", "err")


def filter_model(state, ref, srcs, cams, src_depths, radius=5, step=1):
    """-> dict over all pixels (row-major): passes {criterion: (truth, decided)} [S,N], ok / okdec [S,N] (all three), live [N]
    (d > 0), count [N] nominal, lo / hi [N]: the counts the kernel may return."""
    h, w, _ = state.shape
    rows, cols = np.divmod(np.arange(h * w), w)
    st = np.asarray(state, dtype=np.float32).astype(F).reshape(-1, 4)
    live = st[:, 0] > 0
    d = np.where(live, st[:, 0], 1.0)
    n = np.where(live[:, None], st[:, 1:], np.array([0.0, 0.0, -1.0]))
    cm = cost_model(ref, srcs, cams, rows, cols, d, n, radius, step)
    gm = geom_model(cams, src_depths, rows, cols, d)
    S, N = cm["c"].shape
    slack = abs(MAXCOST32 - PR.FILTER_MAX_COST)
    below = le(cm["craw"], PR.FILTER_MAX_COST, slack)
    ct = cm["valid"] & below[0]
    cd = np.where(cm["vdec"], ~cm["valid"] | below[1], below[1] & ~below[0])
    cmin = math.cos(math.radians(PR.FILTER_MIN_TRI_DEG))
    ang = le(cm["cos"], cmin, abs(COS3_32 - cmin))
    eE = E(gm["e"], gm["eb"])
    eb = le(eE, PR.FILTER_MAX_ERR)
    et = eb[0]
    ed = gm["dec"] & (gm["exact3"] | eb[1])
    parts = dict(cost=(ct, cd), angle3=ang, err=(et, ed))
    ok, okdec = combine(list(parts.values()))
    ok, okdec = ok & live[None], okdec | ~live[None]
    lo = (ok & okdec).sum(0)
    hi = lo + (~okdec).sum(0)
    return dict(passes=parts, ok=ok, okdec=okdec, live=live, count=ok.sum(0), lo=lo, hi=hi, cm=cm, gm=gm)


# ---------------------------------------------------------------------------------------------------------------------------
# candidates
# ---------------------------------------------------------------------------------------------------------------------------
def _random_E(kinv_m, rows, cols, w, dmin, dmax, seed, view, iteration, colour):
    pix = rows.astype(np.int64) * w + cols
    ud = E(PR.pm_uniform(seed, view, pix, iteration, colour, PR.SLOT_RDEPTH))
    uz = E(PR.pm_uniform(seed, view, pix, iteration, colour, PR.SLOT_RZ))
    ua = E(PR.pm_uniform(seed, view, pix, iteration, colour, PR.SLOT_RAZ))
    lo, hi = 1.0 / E(dmax), 1.0 / E(dmin)
    d = 1.0 / (lo + ud * (hi - lo))
    z = 1.0 - 2.0 * uz
    r = sqrt(clamp(1.0 - z * z, 0.0, np.inf))
    sa, ca = esincos(const(2.0 * math.pi, np.float32(6.283185307179586)) * ua)
    n = [r * ca, r * sa, z]
    m = kinv_m
    flip = gt(n[0] * m[0] + n[1] * m[1] + n[2] * m[2], 0.0)
    sgn = np.where(flip[0], -1.0, 1.0)
    return d, [E(sgn * x.v, x.e) for x in n], flip[1]


def _perturb_E(kinv_m, rows, cols, w, cur, dmin, dmax, delta, theta, seed, view, iteration, colour):
    pix = rows.astype(np.int64) * w + cols
    up = E(PR.pm_uniform(seed, view, pix, iteration, colour, PR.SLOT_PHI))
    ua = E(PR.pm_uniform(seed, view, pix, iteration, colour, PR.SLOT_ALPHA))
    ud = E(PR.pm_uniform(seed, view, pix, iteration, colour, PR.SLOT_DEPTH))
    nx, ny, nz = (E(cur[:, 1 + i]) for i in range(3))
    ax = np.abs(cur[:, 1]) < float(np.float32(0.9))
    zero = E(np.zeros(len(rows)))
    pick = lambda a, b: E(np.where(ax, a.v, b.v), np.where(ax, a.e, b.e))
    e1 = [pick(zero, -nz), pick(nz, zero), pick(-ny, nx)]
    il = 1.0 / sqrt(e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2])
    e1 = [x * il for x in e1]
    e2 = [ny * e1[2] - nz * e1[1], nz * e1[0] - nx * e1[2], nx * e1[1] - ny * e1[0]]
    phi = const(theta, np.float32(theta)) * up
    sa, ca = esincos(const(2.0 * math.pi, np.float32(6.283185307179586)) * ua)
    sp, cp = esincos(phi)
    p = [cp * c + sp * (ca * a + sa * b) for c, a, b in zip((nx, ny, nz), e1, e2)]
    ip = 1.0 / sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2])
    p = [x * ip for x in p]
    m = kinv_m
    face = lt(p[0] * m[0] + p[1] * m[1] + p[2] * m[2], 0.0)
    p = [E(np.where(face[0], a.v, b.v), np.where(face[0], a.e, 0.0)) for a, b in zip(p, (nx, ny, nz))]
    lo, hi = 1.0 / E(dmax), 1.0 / E(dmin)
    inv = 1.0 / E(cur[:, 0]) + (2.0 * ud - 1.0) * const(delta, np.float32(delta)) * (hi - lo)
    inv = E(np.clip(inv.v, lo.v, hi.v), inv.e + np.maximum(lo.e, hi.e))
    return 1.0 / inv, p, face[1]


def candidate_model(state, cams, rows, cols, dmin, dmax, delta, theta, seed, view, iteration, colour):
    """-> dict: cand [11,N,4] the rule's candidates (0 where skipped), cb [11,N,4] per-element bounds, live / ldec [11,N] (the depth
    range test of 1-8), cdec [11,N] the candidate's own branch decided (9: faces the camera, 10: the flip)."""
    h, w, _ = state.shape
    st = np.asarray(state, dtype=np.float32).astype(F)
    N = len(rows)
    kinv = _kinv(cams)
    col, row = E(cols.astype(F)), E(rows.astype(F))
    m = [kinv[3 * i] * col + kinv[3 * i + 1] * row + kinv[3 * i + 2] for i in range(3)]
    dmin, dmax = float(np.float32(dmin)), float(np.float32(dmax))
    cand, cb = np.zeros((PR.NUM_CAND, N, 4)), np.zeros((PR.NUM_CAND, N, 4))
    live, ldec, cdec = (np.ones((PR.NUM_CAND, N), bool) for _ in range(3))
    cur = st[rows, cols]
    cand[0] = cur
    for k, (dr, dc) in enumerate(PR.NEIGHBOURS, start=1):
        qr, qc = rows + dr, cols + dc
        inside = (qr >= 0) & (qr < h) & (qc >= 0) & (qc < w)
        q = st[np.clip(qr, 0, h - 1), np.clip(qc, 0, w - 1)]
        fq, fr = E(qc.astype(F)), E(qr.astype(F))
        qn = [E(q[:, 1 + i]) for i in range(3)]
        Q = [E(q[:, 0]) * (kinv[3 * i] * fq + kinv[3 * i + 1] * fr + kinv[3 * i + 2]) for i in range(3)]
        dd = (qn[0] * Q[0] + qn[1] * Q[1] + qn[2] * Q[2]) / (qn[0] * m[0] + qn[1] * m[1] + qn[2] * m[2])
        rng = combine([ge(dd, dmin), le(dd, dmax)])
        lv = inside & rng[0]
        live[k], ldec[k] = lv, ~inside | rng[1]
        with np.errstate(all="ignore"):
            cand[k, :, 0] = np.where(lv, dd.v, 0.0)
            cb[k, :, 0] = np.where(lv, np.where(np.isfinite(dd.e), dd.e, np.inf), 0.0)
        cand[k, :, 1:] = np.where(lv[:, None], q[:, 1:], 0.0)
    d9, n9, dec9 = _perturb_E(m, rows, cols, w, cur, dmin, dmax, delta, theta, seed, view, iteration, colour)
    d10, n10, dec10 = _random_E(m, rows, cols, w, dmin, dmax, seed, view, iteration, colour)
    for k, (dk, nk, deck) in ((9, (d9, n9, dec9)), (10, (d10, n10, dec10))):
        cand[k, :, 0], cb[k, :, 0] = dk.v, dk.e
        for i in range(3):
            cand[k, :, 1 + i], cb[k, :, 1 + i] = nk[i].v, nk[i].e
        cdec[k] = deck
    return dict(cand=cand, cb=cb + SLOP64 * (1 + np.abs(cand)), live=live, ldec=ldec, cdec=cdec)


def init_model(h, w, cams, dmin, dmax, seed, view):
    rows, cols = np.divmod(np.arange(h * w), w)
    kinv = _kinv(cams)
    col, row = E(cols.astype(F)), E(rows.astype(F))
    m = [kinv[3 * i] * col + kinv[3 * i + 1] * row + kinv[3 * i + 2] for i in range(3)]
    d, n, dec = _random_E(m, rows, cols, w, float(np.float32(dmin)), float(np.float32(dmax)), seed, view, PR.INIT_ITERATION, 0)
    v = np.stack([d.v] + [x.v for x in n], -1)
    e = np.stack([d.e] + [x.e for x in n], -1)
    return v.reshape(h, w, 4), (e + SLOP64 * (1 + np.abs(v))).reshape(h, w, 4), dec.reshape(h, w)


# ---------------------------------------------------------------------------------------------------------------------------
# checks: each returns {name: (violations, checked, worst |got - ref| / bound)}; a test asserts violations == 0
# ---------------------------------------------------------------------------------------------------------------------------
def _ratio(diff, bound, mask):
    if not mask.any():
        return 0, 0, 0.0
    with np.errstate(all="ignore"):
        r = np.where(bound > 0, diff / np.where(bound > 0, bound, 1.0), np.where(diff > 0, np.inf, 0.0))[mask]
    r = np.where(np.isnan(r), np.inf, r)
    return int((r > 1.0).sum()), int(mask.sum()), float(r.max())


def topk_own(c, e, top_k):
    """The kernel's own aggregate from its own per-source outputs, in fp32 in its order: ascending sum of the top_k smallest,
    divided by top_k.  -> (value [N] fp32, allowance [N]): bit-exact for the photometric aggregate; the geometric one may
    contract c + 0.3 e into one fma, two roundings of the largest value."""
    f = np.float32
    v = np.asarray(c, dtype=f)
    tol = np.zeros(v.shape[1])
    if e is not None:
        v = (v + f(PR.GEOM_LAMBDA) * np.minimum(np.asarray(e, dtype=f), f(PR.GEOM_EMAX))).astype(f)
        tol = 2 * U * np.abs(v.astype(F)).max(0)
    srt = np.sort(v, axis=0)[:top_k]
    acc = np.zeros(v.shape[1], dtype=f)
    for i in range(top_k):
        acc = (acc + srt[i]).astype(f)
    return (acc / f(top_k)).astype(f), tol


def check_cost(cm, gm, top_k, got_c, got_e, got_agg):
    """got_c [S,N], got_e [S,N] or None, got_agg [N] (fp32 values) against the models."""
    res = {}
    gc = np.asarray(got_c, dtype=F)
    flag = cm["vdec"]
    res["flag"] = (int(((gc == 2.0) != ~cm["valid"])[flag].sum()), int(flag.sum()), 0.0)
    both = flag & cm["valid"]
    res["cost"] = _ratio(np.abs(gc - cm["c"]), cm["cb"] * SCALE["cost"], both)
    if gm is not None:
        ge_ = np.asarray(got_e, dtype=F)
        ex = gm["dec"] & gm["exact3"]
        res["err3"] = (int((ge_ != PR.GEOM_EMAX)[ex].sum()), int(ex.sum()), 0.0)
        res["err"] = _ratio(np.abs(ge_ - gm["e"]), gm["eb"] * SCALE["err"], gm["dec"] & ~gm["exact3"])
    own, tol = topk_own(got_c, got_e if gm is not None else None, top_k)
    ga = np.asarray(got_agg, dtype=F)
    res["topk"] = (int((np.abs(ga - own.astype(F)) > tol).sum()), ga.size, 0.0)
    agg, ab, _ = aggregate_model(cm, gm, top_k)
    res["agg"] = _ratio(np.abs(ga - agg), ab * SCALE["agg"], np.ones(ga.shape, bool))
    return res


def check_candidates(cdm, got_cand):
    """got_cand [N,11,4] of the colour's pixels."""
    g = np.asarray(got_cand, dtype=F).transpose(1, 0, 2)
    skip_k = (g == 0).all(-1)
    res = {"live": (int((skip_k != ~cdm["live"])[cdm["ldec"]].sum()), int(cdm["ldec"].sum()), 0.0)}
    chk = (cdm["ldec"] & cdm["live"] & cdm["cdec"] & ~skip_k)[..., None] & np.ones(4, bool)
    with np.errstate(all="ignore"):
        same = (g == cdm["cand"]) | (np.isnan(g) & np.isnan(cdm["cand"]))          # NaN and inf hypotheses pass through as they are
        res["cand"] = _ratio(np.where(same, 0.0, np.abs(g - cdm["cand"])), cdm["cb"] * SCALE["cand"], chk)
    return res


def check_choice(got_cand, got_choice, agg_of):
    """Regret and tie rule at every pixel of the colour.  got_cand [N,11,4] fp32, got_choice [N]; ``agg_of(k, idx, hyp)`` -> (the
    float64 aggregated cost, its bound) of the kernel's own candidate k at the pixels idx.  -> results and the share of pixels
    whose best two reference costs are separated by more than their bounds (where the index itself is checked)."""
    g = np.asarray(got_cand, dtype=np.float32)
    N = g.shape[0]
    live = ~(g == 0).all(-1)
    live[:, 0] = True
    agg = np.full((PR.NUM_CAND, N), np.inf)
    bnd = np.zeros((PR.NUM_CAND, N))
    for k in range(PR.NUM_CAND):
        idx = np.nonzero(live[:, k])[0]
        if len(idx):
            agg[k, idx], bnd[k, idx] = agg_of(k, idx, g[idx, k])
    ch = np.asarray(got_choice).astype(np.int64)
    ar = np.arange(N)
    res = {"choice_live": (int((~live[ar, ch]).sum()), N, 0.0)}
    best = np.argmin(agg, axis=0)
    regret = agg[ch, ar] - agg[best, ar]
    room = (bnd[ch, ar] + bnd[best, ar]) * SCALE["regret"]
    res["regret"] = _ratio(regret, room, np.ones(N, bool))
    # ties: among the kernel's own bit-identical candidates the lowest index wins
    bits = np.ascontiguousarray(g).view(np.uint32).reshape(N, PR.NUM_CAND, 4)
    same = (bits == bits[ar, ch][:, None]).all(-1) & live
    res["tie"] = (int((np.argmax(same, axis=1) != ch).sum()), N, 0.0)
    # where every other candidate is further from the best than the two bounds, the index is the reference's
    with np.errstate(all="ignore"):
        sep = (agg - agg[best, ar][None] > (bnd + bnd[best, ar][None]) * SCALE["regret"]) | (np.arange(PR.NUM_CAND)[:, None] == best[None])
    sure = sep.all(0)
    res["index"] = (int((ch != best)[sure].sum()), int(sure.sum()), 0.0)
    return res, float(sure.mean())


def check_filter(fm, state, got_depth, got_normal, got_count):
    st = np.asarray(state, dtype=np.float32).reshape(-1, 4)
    gd, gn, gc = np.asarray(got_depth).reshape(-1), np.asarray(got_normal).reshape(-1, 3), np.asarray(got_count).reshape(-1)
    res = {"range": (int(((gc < fm["lo"]) | (gc > fm["hi"])).sum()), gc.size, 0.0)}
    alldec = fm["okdec"].all(0)
    res["count"] = (int((gc != fm["count"])[alldec].sum()), int(alldec.sum()), 0.0)
    keep = gc >= PR.FILTER_MIN_CONSISTENT
    bits = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    bad = np.where(keep, bits(gd) != bits(st[:, 0]), bits(gd) != 0)
    badn = np.where(keep[:, None], bits(gn) != bits(st[:, 1:]), bits(gn) != 0).any(1)
    res["kept_bits"] = (int((bad | badn).sum()), gc.size, 0.0)
    res["dead"] = (int((keep & ~(st[:, 0] > 0)).sum()), int((~(st[:, 0] > 0)).sum()), 0.0)
    return res


def failures(res):
    return {k: v for k, v in res.items() if v[0]}


def fmt(tag, res):
    return f"[pm-ref] {tag}: " + ", ".join(f"{k} {v[0]}/{v[1]}" + (f" r={v[2]:.3g}" if v[2] else "") for k, v in res.items())
