"""Float64 reference of the softmax regression family (pscv_softargmin, pscv_softargmin_window and the fused siblings that are
tested against them).  numpy on the CPU, no project imports.

Semantics are those of ``torch.softmax`` over the plane axis: a ``-inf`` logit weighs zero; a column that is all ``-inf`` or that
holds ``+inf`` or NaN is NaN in every output.  Reference lines replaced (fdarmon/wild_deep_mvs): models/MVSNet/model.py:207-215,
models/MVSNet/module.py:174-178, models/VisMVSNet/nn_utils.py:453-470.

The caller rounds the logits to their storage type first, so the reference sees what the kernel reads."""
import numpy as np


def _f64(a):
    if hasattr(a, "detach"):
        a = a.detach().cpu().double().numpy()
    return np.asarray(a, dtype=np.float64)


def _planes(planes, shape):
    """[B,D] or [B,D,h,w] -> [B,D,h,w] (broadcast view)."""
    p = _f64(planes)
    if p.ndim == 2:
        p = p[:, :, None, None]
    return np.broadcast_to(p, shape)


def _column_stats(logits):
    """max [B,h,w], e = exp(l - max) [B,D,h,w]; a bad column (all -inf, +inf, NaN) is NaN throughout."""
    with np.errstate(invalid="ignore", over="ignore"):
        m = logits.max(axis=1)
        bad = ~np.isfinite(m)                       # NaN (np.max propagates it), +inf, or -inf = every plane -inf
        ms = np.where(bad, 0.0, m)
        e = np.exp(logits - ms[:, None])
        e = np.where(bad[:, None], np.nan, e)
        m = np.where(bad & ~np.isneginf(m), np.nan, m)
    return m, e, bad


class Ref:
    """All outputs of one softargmin call in float64.  ``index`` carries ``index_offset``; ``lidx`` is local to the logit block."""

    def __init__(self, logits, planes=None, index_offset=0):
        l = _f64(logits)
        assert l.ndim == 4
        self.logits = l
        self.B, self.D, self.h, self.w = l.shape
        self.offset = int(index_offset)
        self.m, self.e, self.bad = _column_stats(l)
        self.z = self.e.sum(axis=1)
        with np.errstate(invalid="ignore", divide="ignore"):
            self.prob = self.e / self.z[:, None]
        self.d = np.arange(self.D, dtype=np.float64).reshape(1, self.D, 1, 1)
        self.lidx = (self.prob * self.d).sum(axis=1)
        self.index = self.lidx + self.offset
        self.planes = None if planes is None else _planes(planes, l.shape)
        self.depth = None if planes is None else (self.prob * self.planes).sum(axis=1)

    # ---- entropy: the reference clamps p to [1e-9, 1] inside the logarithm (nn_utils.py:469-470)
    def entropy(self, clamp=True):
        p = self.prob
        with np.errstate(invalid="ignore", divide="ignore"):
            lg = np.log(np.clip(p, 1e-9, 1.0)) if clamp else np.where(p > 0, np.log(np.where(p > 0, p, 1.0)), 0.0)
            ent = -(p * lg).sum(axis=1)
        return np.where(self.bad, np.nan, ent)

    # ---- confidences at a GIVEN local index (so the alternatives of ``fragile`` use the same code)
    def _conf0_at(self, i):
        """sum of p over planes i-1 .. i+2, zero padded; i integer [B,h,w]."""
        c = np.zeros(i.shape)
        for k in (-1, 0, 1, 2):
            dd = i + k
            ok = (dd >= 0) & (dd < self.D)
            g = np.take_along_axis(self.prob, np.clip(dd, 0, self.D - 1)[:, None], axis=1)[:, 0]
            c = c + np.where(ok, g, 0.0)
        return c

    def _trunc(self):
        return np.trunc(np.where(self.bad, 0.0, self.lidx)).astype(np.int64)

    def conf0(self):
        """planes i-1 .. i+2 around i = trunc(index - offset), zero padded (model.py:211-215)."""
        return np.where(self.bad, np.nan, self._conf0_at(self._trunc()))

    def _mask1(self, window):
        lid = np.where(self.bad, 0.0, self.lidx)
        return np.abs(self.d - lid[:, None]) <= window

    def conf1(self, window):
        """sum of p over planes with |d - (index - offset)| <= window (nn_utils.py:464-465)."""
        return np.where(self.bad, np.nan, (self.prob * self._mask1(window)).sum(axis=1))

    def conf(self, mode, window=2.0):
        return self.conf0() if mode == 0 else self.conf1(window)

    def fragile(self, mode, eps, window=2.0):
        """(mask, alts): where the float64 local index lies within ``eps`` of the confidence's discontinuity, ``alts`` lists the
        values on the other side of it -- mode 0: the window around the neighbouring integer; mode 1: the boundary plane(s) toggled,
        once for an index a little higher and once for one a little lower.  Elsewhere every alternative equals the reference value.
        ``eps`` is the tolerance of the kernel's index, so a kernel within that tolerance gives the reference or an alternative."""
        lid = np.where(self.bad, 0.0, self.lidx)
        if mode == 0:
            i = self._trunc()
            frac = lid - i
            up = frac >= 1.0 - eps                       # the kernel's index may reach i + 1
            dn = (frac <= eps) & (i >= 1)                # ... or fall below i (trunc of a negative local index stays 0)
            alt = self._conf0_at(np.where(up, i + 1, np.where(dn, i - 1, i)))
            mask = up | dn
            return mask & ~self.bad, [np.where(self.bad, np.nan, alt)]
        dist = np.abs(self.d - lid[:, None])
        edge = np.abs(dist - window) <= eps              # planes that sit on the window's edge
        inside = dist <= window
        # an index error moves every plane's distance the same way along d: planes on the lower edge and on the upper edge toggle
        # oppositely.  The alternatives: index a little higher (lower-edge planes leave, upper-edge planes enter) and a little lower.
        lower = edge & (self.d < lid[:, None])
        upper = edge & (self.d > lid[:, None])
        hi = (inside & ~lower) | upper
        lo = (inside & ~upper) | lower
        # and, where a lower and an upper plane sit on the edge together (2 * window apart: an index exactly between them), both in
        alts = [(self.prob * sel).sum(axis=1) for sel in (hi, lo, inside | edge)]
        mask = edge.any(axis=1) & ~self.bad
        nan = np.where(self.bad, np.nan, 0.0)
        return mask, [a + nan for a in alts]

    def partials(self):
        """[B,4,h,w]: (max, sum e, sum e * depth, sum e * index) with e = exp(l - max); the index carries the offset.  A shard whose
        planes are all -inf has max -inf and zero sums."""
        m = np.where(self.bad & np.isneginf(self.m), -np.inf, self.m)
        empty = np.isneginf(m)
        e = np.where(empty[:, None], 0.0, self.e)
        sd = (e * self.planes).sum(axis=1) if self.planes is not None else np.zeros_like(m)
        si = (e * (self.d + self.offset)).sum(axis=1)
        return np.stack([m, e.sum(axis=1), sd, si], axis=1)


def merge(parts):
    """Log-sum-exp merge of shard partials [B,4,h,w] -> dict(max, z, depth, index).  A shard whose max is -inf contributes nothing."""
    parts = [_f64(p) for p in parts]
    M = parts[0][:, 0]
    for p in parts[1:]:
        M = np.maximum(M, p[:, 0])
    Z = np.zeros_like(M); SD = np.zeros_like(M); SI = np.zeros_like(M)
    with np.errstate(invalid="ignore", divide="ignore"):
        for p in parts:
            live = ~np.isneginf(p[:, 0])
            f = np.where(live, np.exp(np.where(live, p[:, 0], 0.0) - np.where(np.isfinite(M), M, 0.0)), 0.0)
            Z = Z + np.where(live, p[:, 1] * f, 0.0)
            SD = SD + np.where(live, p[:, 2] * f, 0.0)
            SI = SI + np.where(live, p[:, 3] * f, 0.0)
        return {"max": M, "z": Z, "depth": SD / Z, "index": SI / Z}


def window_shard(logits, M, Z, index, window, index_offset):
    """What pscv_softargmin_window owes for one shard: sum over its planes d with |d + offset - index| <= window of exp(l_d - M) / Z."""
    l = _f64(logits)
    M, Z, index = _f64(M), _f64(Z), _f64(index)
    d = np.arange(l.shape[1], dtype=np.float64).reshape(1, -1, 1, 1) + index_offset
    with np.errstate(invalid="ignore", over="ignore"):
        p = np.exp(l - M[:, None]) / Z[:, None]
    return (p * (np.abs(d - index[:, None]) <= window)).sum(axis=1)
