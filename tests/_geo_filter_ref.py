"""Float64 reference of the geometric-consistency filter, pscv_geo_filter (csrc/geo_filter.hip), per (source, pixel) pair and per
criterion, written with numpy from the rules of oracle/filtering.py.  It never imports ``wild_deep_mvs_amd.ops``: the camera blocks
[V,30] (K, fp32 K^-1, R, t -- what ``ops.geo_filter_cams`` hands the kernel) come in as an array, ``cam_blocks`` below builds the same.

For every pair the reference gives three DECISIONS -- ``disp`` (reprojection error), ``depth`` (relative depth difference and its two
sign tests), ``tri`` (triangulation angle) -- their conjunction ``geo``, and whether each is DECIDED: each tested inequality is
evaluated over the interval [value - e, value + e] of its inputs, e = k 2^-24 U, and a decision is decided when both ends agree.

Error units (the convention of tests/_photo_ref.py).  ``EV`` carries a value and a unit U built from ABSOLUTE values; every fp32
operation of the kernel's chain adds the magnitude of its own result once per rounding, and what its operands carry is propagated to
first order:  a 3-term dot product adds 3 sum_k |m_k v_k| (product + two fused multiply-adds; the unfused order, three products and
two sums, is bounded by the same 3), a sum / product / quotient / square root adds |result|, the bilinear sample adds
7 sum_k |w_k v_k| (a weight is two differences and a product, then the product and sum of the fused accumulation) and
U_ix |dV/dix| + U_iy |dV/diy| with the larger one-sided slope inside the position margin.  The non-linear steps are NOT linearised:
q / z' is bounded from the interval magnitudes of q and z' (so a z' that straddles 0 still gives a lower bound of the reprojection
error), |z' - d| - max(z', d) thr is convex in z' and evaluated at the interval ends (and at z' = d inside), acos is evaluated at the
two ends of the clamped cosine interval.  A pair whose sample position is uncertain by more than a quarter texel, or whose source depth
z_i sits within its error of the 1e-6 clamp, is undecided in everything that depends on the sample.

The constants k.  U counts every rounding of the kernel's own path once, so k = 1 is the first-order bound of the kernel AND of any
evaluation with no more roundings per step (the oracle's unfused GEMM rows).  What k has to cover beyond 1:
  K_CHAIN = 2   second-order terms (products of two relative errors of <= 40 roundings: (40 2^-24)^2, far below one unit) and the
                difference between the kernel's and the oracle's order in the scalar steps that are NOT dot products: the oracle
                divides by (size - 1) after 2 u, the kernel the same; the oracle's grid_sample computes ((g + 1) size - 1) / 2
                as (g + 1) (size / 2) - 0.5, the same count of roundings on other partial results, each bounded by the same
                magnitudes; doubling the unit covers a step whose partial result is up to twice the one counted.
  K_ANGLE = 6   relative, on the angle: acosf is accurate to 2 ulp (1 unit is half an ulp: 4), the division by the fp32 pi
                (off from pi by 0.47 units) and the product with 180 (1 + 1, rounded up with the 0.47 to 2).  The cosine itself
                carries K_CHAIN U like everything else.
  K_TEST = 4    relative, on each side of a tested inequality: the subtraction, the product with the threshold, the two squares,
                their sum and the square root round once each on the kernel's path, at most four on either side.
None of the three is measured on a GPU.

Non-finite depths.  NaN or inf in the reference map or in a tap of the sample propagate through the float64 evaluation exactly as
through the kernel's (0 inf = NaN, inf - inf = NaN; no product or sum here overflows fp32 for depths below 1e15): every comparison
with NaN is false, so such a pair is decided (all three counted decisions false) whenever the tap footprint itself is certain.  The
kernel's fminf / fmaxf drop a NaN cosine where ATen's clamp keeps it: ``tri`` is left undecided there (it is never observable:
``depth`` is false)."""
import numpy as np

EPS = 2.0 ** -24
K_CHAIN, K_ANGLE, K_TEST = 2.0, 6.0, 4.0
ZMIN = float(np.float32(1e-6))
NMIN = float(np.float32(1e-12))
PI32 = float(np.float32(np.pi))
POS_MARGIN_MAX = 0.25              # texels: beyond this the sample is not bounded, the pair is undecided
CRITERIA = ("disp", "depth", "tri")
VARIANTS = (None, "align_corners", "norm_size", "no_eps", "min_for_max", "radians")
F = np.float64


class EV:
    """value + first-order error unit (units of one fp32 rounding of an O(1) number), numpy float64 arrays."""

    def __init__(self, v, e=None):
        self.v = np.asarray(v, dtype=F)
        self.e = np.zeros_like(self.v) if e is None else np.asarray(e, dtype=F)

    @staticmethod
    def lift(x):
        return x if isinstance(x, EV) else EV(x)

    def __add__(self, o):
        o = EV.lift(o)
        v = self.v + o.v
        return EV(v, self.e + o.e + np.abs(v))
    __radd__ = __add__

    def __sub__(self, o):
        o = EV.lift(o)
        v = self.v - o.v
        return EV(v, self.e + o.e + np.abs(v))

    def __mul__(self, o):
        o = EV.lift(o)
        v = self.v * o.v
        # (0 e = 0 even where e is inf / NaN: an exact zero factor with no unit of its own carries nothing)
        a = np.where((o.v == 0) & (o.e == 0), 0.0, self.e * np.abs(o.v))
        b = np.where((self.v == 0) & (self.e == 0), 0.0, o.e * np.abs(self.v))
        return EV(v, a + b + np.abs(v))
    __rmul__ = __mul__

    def __truediv__(self, o):
        o = EV.lift(o)
        v = self.v / o.v
        return EV(v, (self.e + np.abs(v) * o.e) / np.abs(o.v) + np.abs(v))

    def scaled(self, c):
        """times a power of two: exact"""
        return EV(self.v * c, self.e * abs(c))

    def sqrt(self):
        v = np.sqrt(self.v)
        return EV(v, np.where(v > 0, self.e / np.where(v > 0, 2.0 * v, 1.0), np.inf) + v)      # (no first order at 0: unbounded)


def _dot3(m, x, y, z):
    t0, t1, t2 = m[0] * x.v, m[1] * y.v, m[2] * z.v
    return EV(t0 + t1 + t2, abs(m[0]) * x.e + abs(m[1]) * y.e + abs(m[2]) * z.e + 3.0 * (np.abs(t0) + np.abs(t1) + np.abs(t2)))


def _mat(M, x, y, z):
    return _dot3(M[0:3], x, y, z), _dot3(M[3:6], x, y, z), _dot3(M[6:9], x, y, z)


def _matT(M, x, y, z):
    return _dot3(M[0::3], x, y, z), _dot3(M[1::3], x, y, z), _dot3(M[2::3], x, y, z)


def _unproject(cam, x, y, d):
    """R^T (d K^-1 (x, y, 1) - t)  with the block's own fp32 K^-1"""
    K, Ki, R, t = cam[0:9], cam[9:18], cam[18:27], cam[27:30]
    a = _mat(Ki, x * d, y * d, d)
    return _matT(R, a[0] - t[0], a[1] - t[1], a[2] - t[2])


def _point(cam, X, Y, Z):
    """K (R X + t)"""
    K, Ki, R, t = cam[0:9], cam[9:18], cam[18:27], cam[27:30]
    c = _mat(R, X, Y, Z)
    return _mat(K, c[0] + t[0], c[1] + t[1], c[2] + t[2])


def cam_blocks(K, R, t):
    """[V,3,3], [V,3,3], [V,3,1] torch fp32 tensors -> float64 [V,30] with the VALUES of ``ops.geo_filter_cams``: the inverse is
    ``torch.inverse`` in fp32, like the oracle's (utils_3D.py:131, 155)."""
    import torch
    K = K.to(torch.float32)
    b = torch.cat((K.reshape(-1, 9), torch.inverse(K).reshape(-1, 9), R.to(torch.float32).reshape(-1, 9), t.to(torch.float32).reshape(-1, 3)), 1)
    return b.double().numpy()


def _taps(src, ix, iy):
    """zero-padded bilinear value V, A = sum |w v|, the two slopes; every in-bounds tap enters whatever its weight (the kernel's
    fused accumulation: 0 NaN = NaN), out-of-bounds taps do not."""
    hs, ws = src.shape
    x0, y0 = np.floor(ix), np.floor(iy)
    ax, ay = ix - x0, iy - y0
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)

    def tap(yy, xx):
        ok = (xx >= 0) & (xx < ws) & (yy >= 0) & (yy < hs)
        return np.where(ok, src[np.clip(yy, 0, hs - 1), np.clip(xx, 0, ws - 1)], 0.0), ok
    (v00, k00), (v01, k01), (v10, k10), (v11, k11) = tap(y0, x0), tap(y0, x0 + 1), tap(y0 + 1, x0), tap(y0 + 1, x0 + 1)
    w00, w01, w10, w11 = (1 - ax) * (1 - ay), ax * (1 - ay), (1 - ax) * ay, ax * ay
    V = v00 * w00 + v01 * w01 + v10 * w10 + v11 * w11
    A = np.abs(v00 * w00) + np.abs(v01 * w01) + np.abs(v10 * w10) + np.abs(v11 * w11)
    sx = np.abs((v01 - v00) * (1 - ay) + (v11 - v10) * ay)
    sy = np.abs((v10 - v00) * (1 - ax) + (v11 - v01) * ax)
    bad = ~(np.isfinite(v00) & np.isfinite(v01) & np.isfinite(v10) & np.isfinite(v11))
    return V, A, sx, sy, bad


def _mag_bounds(x, k=K_CHAIN):
    """|x| in [lo, hi] and whether the sign of x is certain"""
    m = k * EPS * x.e
    a = np.abs(x.v)
    return np.maximum(a - m, 0.0), a + m, a > m


def _abs_quot_minus(q, z, c):
    """bounds of |q / z - c| (c >= 0 exact) from the interval magnitudes of q and z; z may straddle 0"""
    qlo, qhi, qs = _mag_bounds(q)
    zlo, zhi, zs = _mag_bounds(z)
    with np.errstate(divide="ignore", invalid="ignore"):
        mlo = np.where(zhi > 0, qlo / np.where(zhi > 0, zhi, 1.0), np.where(qlo > 0, np.inf, 0.0)) * (1.0 - 2.0 * EPS)
        mhi = np.where(zlo > 0, qhi / np.where(zlo > 0, zlo, 1.0), np.inf) * (1.0 + 2.0 * EPS)
    sure = qs & zs
    s = np.sign(q.v) * np.sign(z.v)
    e1, e2 = s * mlo - c, s * mhi - c
    lo_s = np.where((e1 <= 0) == (e2 <= 0), np.minimum(np.abs(e1), np.abs(e2)), 0.0)
    hi_s = np.maximum(np.abs(e1), np.abs(e2))
    lo = np.where(sure, lo_s, np.maximum(mlo - c, 0.0))
    hi = np.where(sure, hi_s, mhi + c)
    return lo, hi


def pairs(depth, src_depth, cams, params, variant=None):
    """depth [h,w], src_depth N x [h_i,w_i] (arrays of fp32 VALUES), cams [N+1,30] (``cam_blocks``), params = (max_reproj_error,
    depth_threshold, min_tri_angle) -> dict of bool [N,h,w] arrays: ``disp``, ``depth``, ``tri``, ``geo`` and ``<name>_decided``.
    ``variant`` plants one error in the nominal evaluation (tests only): see VARIANTS."""
    assert variant in VARIANTS, variant
    depth = np.asarray(depth, dtype=F)
    cams = np.asarray(cams, dtype=F)
    h, w = depth.shape
    N = len(src_depth)
    thr_disp, thr_depth, thr_tri = (float(np.float32(p)) for p in params)
    ys, xs = np.meshgrid(np.arange(h, dtype=F), np.arange(w, dtype=F), indexing="ij")
    xs, ys, d = xs.reshape(-1), ys.reshape(-1), depth.reshape(-1)
    out = {k: np.zeros((N, h * w), dtype=bool) for k in CRITERIA + ("geo",)}
    out.update({k + "_decided": np.zeros((N, h * w), dtype=bool) for k in CRITERIA + ("geo",)})
    zmin_back = 0.0 if variant == "no_eps" else ZMIN
    with np.errstate(all="ignore"):
        c0 = cams[0]
        X, Y, Z = _unproject(c0, EV(xs), EV(ys), EV(d))
        t0 = c0[27:30]
        cw0 = _matT(c0[18:27], EV(t0[0]), EV(t0[1]), EV(t0[2]))
        r1 = (X + cw0[0], Y + cw0[1], Z + cw0[2])
        n1 = (r1[0] * r1[0] + r1[1] * r1[1] + r1[2] * r1[2]).sqrt()
        d_bad = ~np.isfinite(d)
        for i in range(N):
            ci = cams[i + 1]
            src = np.asarray(src_depth[i], dtype=F)
            hs, ws = src.shape
            px, py, pz = _point(ci, X, Y, Z)
            mz = K_CHAIN * EPS * pz.e
            front = pz.v - mz > 0                                  # z_i > 0 certainly
            behind = pz.v + mz <= 0
            clamped = pz.v + mz <= ZMIN                            # max(z_i, 1e-6) is 1e-6 certainly: exact
            zc = EV(np.maximum(pz.v, ZMIN), np.where(clamped, 0.0, pz.e))
            unknown = ~clamped & (K_CHAIN * EPS * zc.e > 0.25 * zc.v)          # the quotient's first order does not hold
            u, v = px / zc, py / zc
            pos = []
            for c, size in ((u, ws), (v, hs)):
                if variant == "align_corners":                     # ((g + 1) / 2) (size - 1)
                    g = c.scaled(2.0) / (size - 1.0) - 1.0
                    pos.append(((g + 1.0).scaled(0.5)) * (size - 1.0))
                elif variant == "norm_size":                       # g = 2 u / size - 1
                    g = c.scaled(2.0) / float(size) - 1.0
                    pos.append(((g + 1.0) * float(size) - 1.0).scaled(0.5))
                else:
                    g = c.scaled(2.0) / (size - 1.0) - 1.0
                    pos.append(((g + 1.0) * float(size) - 1.0).scaled(0.5))
            ix, iy = pos
            mx, my = K_CHAIN * EPS * ix.e, K_CHAIN * EPS * iy.e
            # V = 0 for ix <= -1 and ix >= ws (every tap outside or weightless); a NaN position fails the kernel's range test
            outside = (ix.v + mx <= -1.0) | (ix.v - mx >= ws) | (iy.v + my <= -1.0) | (iy.v - my >= hs) | np.isnan(ix.v) | np.isnan(iy.v)
            unknown |= ~outside & ((mx > POS_MARGIN_MAX) | (my > POS_MARGIN_MAX))
            sx_ = np.where(outside | unknown, 0.0, ix.v)
            sy_ = np.where(outside | unknown, 0.0, iy.v)
            V, A, sxm, sym, tap_bad = _taps(src, sx_, sy_)
            may_bad = tap_bad.copy()
            for dx, dy in ((-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (-1, 1), (1, -1), (1, 1)):
                _, _, a, b, bad = _taps(src, sx_ + dx * np.minimum(mx, POS_MARGIN_MAX), sy_ + dy * np.minimum(my, POS_MARGIN_MAX))
                sxm, sym = np.fmax(sxm, a), np.fmax(sym, b)
                may_bad |= bad
            footprint_sure = (np.floor(sx_ - mx) == np.floor(sx_ + mx)) & (np.floor(sy_ - my) == np.floor(sy_ + my))
            live = ~outside & ~unknown
            sample_bad = live & tap_bad & footprint_sure           # the sample is NaN / inf certainly
            unknown |= live & may_bad & ~sample_bad                # it may or may not be
            dw = EV(np.where(outside, 0.0, V), np.where(outside | sample_bad, 0.0, ix.e * sxm + iy.e * sym + 7.0 * A))
            Xr, Yr, Zr = _unproject(ci, u, v, dw)
            qx, qy, qz = _point(c0, Xr, Yr, Zr)
            zr = qz + zmin_back
            nonfinite = d_bad | sample_bad                         # decided by propagation: the nominal evaluation IS the kernel's

            # ---- disp: |q_xy / z' - (x, y)| < max_reproj_error
            rx, ry = qx.v / zr.v - xs, qy.v / zr.v - ys
            disp = np.sqrt(rx * rx + ry * ry) < thr_disp
            xl, xh = _abs_quot_minus(qx, zr, xs)
            yl, yh = _abs_quot_minus(qy, zr, ys)
            elo = np.sqrt(xl * xl + yl * yl) * (1.0 - K_TEST * EPS)
            ehi = np.sqrt(xh * xh + yh * yh) * (1.0 + K_TEST * EPS)
            disp_dec = (ehi < thr_disp) | (elo >= thr_disp)
            disp_dec = np.where(nonfinite, True, disp_dec & ~unknown)

            # ---- depth: |z' - d| < max(z', d) thr  and  z' > 0  and  z_i > 0
            pick = np.minimum if variant == "min_for_max" else np.maximum
            f = lambda z: np.abs(z - d) - pick(z, d) * thr_depth
            slack = lambda z: K_TEST * EPS * (np.abs(z - d) + np.abs(pick(z, d)) * thr_depth)
            dep = (f(zr.v) < 0) & (zr.v > 0) & (pz.v > 0)
            mr = K_CHAIN * EPS * zr.e
            zl, zh = zr.v - mr, zr.v + mr
            inside = (zl <= d) & (d <= zh)
            fmax = np.maximum(f(zl) + slack(zl), f(zh) + slack(zh))
            fmin = np.minimum(f(zl) - slack(zl), f(zh) - slack(zh))
            fmin = np.where(inside, np.minimum(fmin, f(d) - slack(d)), fmin)
            dep_true = (fmax < 0) & (zl > 0) & front
            dep_false_sample = (fmin >= 0) | (zh <= 0)             # needs the sample
            dep_dec = np.where(nonfinite, True, behind | ((dep_true | dep_false_sample) & ~unknown))

            # ---- tri: angle(X - c_0, X - c_i) > min_tri_angle, degrees
            ti = ci[27:30]
            cwi = _matT(ci[18:27], EV(ti[0]), EV(ti[1]), EV(ti[2]))
            r2 = (X + cwi[0], Y + cwi[1], Z + cwi[2])
            n2 = (r2[0] * r2[0] + r2[1] * r2[1] + r2[2] * r2[2]).sqrt()
            dot = r1[0] * r2[0] + r1[1] * r2[1] + r1[2] * r2[2]
            n1c, n2c = EV(np.maximum(n1.v, NMIN), n1.e), EV(np.maximum(n2.v, NMIN), n2.e)
            cos = dot / n1c / n2c
            norm_ok = (K_CHAIN * EPS * n1c.e < 0.25 * n1c.v) & (K_CHAIN * EPS * n2c.e < 0.25 * n2c.v)
            mc = K_CHAIN * EPS * cos.e
            clo = np.where(norm_ok, np.clip(cos.v - mc, -1.0, 1.0), -1.0)
            chi = np.where(norm_ok, np.clip(cos.v + mc, -1.0, 1.0), 1.0)
            scale = 1.0 if variant == "radians" else 180.0 / PI32
            ang = np.arccos(np.clip(cos.v, -1.0, 1.0)) * scale
            tri = ang > thr_tri
            alo = np.arccos(chi) * scale * (1.0 - K_ANGLE * EPS)
            ahi = np.arccos(clo) * scale * (1.0 + K_ANGLE * EPS)
            tri_dec = ((alo > thr_tri) | (ahi <= thr_tri)) & np.isfinite(cos.v)

            geo = disp & dep & tri
            geo_dec = (disp_dec & dep_dec & tri_dec) | (disp_dec & ~disp) | (dep_dec & ~dep) | (tri_dec & ~tri)
            if variant is None:                                    # the intervals contain the nominal value
                assert not np.any(~nonfinite & disp_dec & (disp != (ehi < thr_disp))), "disp interval"
                assert not np.any(~nonfinite & ~behind & dep_dec & (dep != dep_true)), "depth interval"
                assert not np.any(behind & dep), "behind"
                assert not np.any(tri_dec & (tri != (alo > thr_tri))), "tri interval"
            for k, val, dec in (("disp", disp, disp_dec), ("depth", dep, dep_dec), ("tri", tri, tri_dec), ("geo", geo, geo_dec)):
                out[k][i], out[k + "_decided"][i] = val, dec
    return {k: a.reshape(N, h, w) for k, a in out.items()}


def undecided_share(r):
    """share of the (source, pixel, criterion) triples that are not decided, and of the conjunction on its own"""
    tri = np.mean([1.0 - r[k + "_decided"].mean() for k in CRITERIA])
    return float(tri), float(1.0 - r["geo_decided"].mean())


def counts(r):
    """[3,h,w] counts in the kernel's order (depth, disp, geo) from the nominal decisions, and whether every source of the pixel is decided"""
    c = np.stack([r[k].sum(0) for k in ("depth", "disp", "geo")]).astype(np.int64)
    dec = np.stack([r[k + "_decided"].all(0) for k in ("depth", "disp", "geo")])
    return c, dec


# ---- the cases of the CPU and GPU tests -------------------------------------------------------------------------------------------------
PARAMS = ((3, (1.0, 0.01, 1.0)), (2, (0.5, 0.005, 3.0)))      # (num_consistent, (max_reproj_error, depth_threshold, min_tri_angle))
RANDOM_SCENES = {"9v-96x128": (9, 96, 128, dict(behind_view=5, half_res_view=2, near_view=7)), "3v-37x53": (3, 37, 53, dict()),
                 "33v-40x48": (33, 40, 48, dict(near_view=1))}


def _resample(m, h, w):
    import torch
    return torch.nn.functional.interpolate(m.view(1, 1, *m.shape), size=(h, w), mode="bilinear", align_corners=False)[0, 0].contiguous()


def make_case(name):
    """-> dict(depth, src_depth, K, R, t) of torch fp32 tensors, view 0 the reference.  The random scenes are the ones of
    tests/test_gpu_filter.py; the others are small edits of the 3-view scene."""
    import torch
    from wild_deep_mvs_amd import synthetic
    if name in RANDOM_SCENES:
        V, H, W, kw = RANDOM_SCENES[name]
        return synthetic.make_filter_scene(V, H, W, seed=V, **kw)
    sc = synthetic.make_filter_scene(3, 37, 53, seed=3)
    K, R, t = sc["K"].clone(), sc["R"].clone(), sc["t"].clone()
    depth, src = sc["depth"].clone(), [s.clone() for s in sc["src_depth"]]
    if name == "one-source":
        K, R, t, src = K[:2], R[:2], t[:2], src[:1]
    elif name == "row-1x300":
        # one row of a 300-wide view of the same plane: a second, ragged workgroup (300 = 256 + 44)
        wide = synthetic.make_filter_scene(3, 8, 300, seed=5)
        K, R, t, src = wide["K"].clone(), wide["R"].clone(), wide["t"].clone(), [s.clone() for s in wide["src_depth"]]
        depth = wide["depth"][0:1].clone().contiguous()          # row y = 0 of the reference map: same camera, h = 1
    elif name == "src-sizes":
        # source 0 rendered at 1.5 x the reference's size, source 1 shrunk to 2 x 2 (intrinsics scaled with the maps)
        for i, (hh, ww) in enumerate(((56, 80), (2, 2))):
            sy, sx = hh / src[i].shape[0], ww / src[i].shape[1]
            src[i] = _resample(src[i], hh, ww)
            K[i + 1, 0] *= sx
            K[i + 1, 1] *= sy
    elif name == "non-finite":
        g = torch.Generator().manual_seed(17)
        for m in [depth] + src:
            idx = torch.randperm(m.numel(), generator=g)[:12]
            flat = m.view(-1)
            flat[idx[:4]] = 0.0
            flat[idx[4:8]] = float("nan")
            flat[idx[8:]] = float("inf")
        depth[5, 7:11] = 0.0
        src[0][10:14, 20:24] = float("nan")
    elif name == "pure-rotation":
        # both sources share the reference's centre c = 0 (t = 0 everywhere): the two rays of a pair are the same vector
        t = torch.zeros_like(t)
        a = 0.005                                                # a quarter texel at this focal length: no sample grazes the rim
        R[1] = torch.tensor([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]], dtype=torch.float32) @ R[0]
        R[2] = R[0].clone()
        K[1], K[2] = K[0].clone(), K[0].clone()
        src[1] = depth.clone()
    elif name == "micro-scale":
        # the same scene shrunk until the back-projection's +1e-6 is a percent of the depth (depths ~ 1e-4)
        s = 2.5e-5
        depth, src, t = depth * s, [m * s for m in src], t * s
    else:
        raise KeyError(name)
    return {"depth": depth.contiguous(), "src_depth": [m.contiguous() for m in src], "K": K, "R": R, "t": t}


GPU_CASES = tuple(RANDOM_SCENES) + ("one-source", "row-1x300", "src-sizes", "non-finite", "pure-rotation", "micro-scale")
UNDECIDED_CAP = 0.01


def reference(case, params):
    sc = case if isinstance(case, dict) else make_case(case)
    cams = cam_blocks(sc["K"], sc["R"], sc["t"])
    return pairs(sc["depth"].numpy(), [s.numpy() for s in sc["src_depth"]], cams, params)
