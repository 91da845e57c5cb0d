"""Float64 reference of one pass of the depth-map fusion (pscv_fuse_depth_pass, csrc/depth_fusion.hip; the rule of INTEGRATION.md
section 2d) with a running error bound per step, the decisions evaluated over their intervals, and the comparison of a pass's
outputs -- the kernel's or the fp32 emulation's (tests/_fusion_emu.py) -- with it.  numpy only; never imports ``ops``.

Inputs are the fp32 numbers the kernel reads: depth maps, camera blocks [N,30] (K, the fp32 K^-1, R, t), and the three thresholds as
``np.float32`` (the C ABI takes them as float).

Error bound (``IV``: value v and an ABSOLUTE bound e of |kernel's value - v|).  Every fp32 operation is correctly rounded (products,
sums, fmaf, and division and sqrtf as the build leaves them: correctly rounded), so a step whose exact result is r returns r (1 + d),
|d| <= 2^-24 (plus 2^-149 should r be subnormal).  A step therefore carries
    e_out = P + 2^-24 (|v| + P) + 2^-149,      P = what its operands' bounds propagate to,
with P taken rigorously, not to first order: a product carries e_a |b| + e_b |a| + e_a e_b, a quotient (e_a + |v| e_b) / (|b| - e_b)
(unbounded when the divisor's interval reaches 0), a square root e_s / sqrt(s) (from |s' - s| / (sqrt s' + sqrt s)), an fmaf counts ONE
rounding.  A step whose operands are exact (e = 0) and whose exact result is an fp32 number counts ZERO: the kernel returns that number.
A division by an exact power of two is a scaling and counts zero as well.  No constant is fitted.

Roundings per helper of csrc/geo_common.h, as coded here:
    mat_vec, matT_vec    3 per component: one product, two fmaf                                              (``_mat``, ``_matT``)
    cam_unproject        2 products (x d, y d) + mat_vec 9 + 3 differences with t + matT_vec 9 = 23           (``_unproject``)
    cam_point            mat_vec 9 + 3 sums with t + mat_vec 9 = 21                                          (``_point``)
    fb_lds[j]            two matT_vec (R^T t: 9 each) + 3 differences (which cancel for a short baseline: their bound is that of the
                         centres, not of the difference) + 3 squares + 2 sums + sqrtf + the product with K[0].  The squares and sums
                         may be contracted into fmaf by the compiler: fewer roundings of partial sums that are no larger (all terms
                         are >= 0), so the unfused count bounds every contraction                            (``_baseline``)
    per (pixel, view j)  a / z, b / z, + 0.5f (two roundings each coordinate), floorf exact;  fb / z, fb / d_j, their difference (3);
                         the neighbour's cam_unproject from exact (q_x, q_y, d_j)
    the mean             the running sums in view order, one rounding per consistent view after the first (0 + X_j is exact), the sum
                         with the pixel's own point, the division by (float)(n + 1); n = 0 adds nothing (X + 0, X / 1 are exact)

Decisions.  Each is evaluated at both ends of its interval and is DECIDED when they agree:
    front    z > 0
    round    which integers floor(a / z + 0.5) and floor(b / z + 0.5) are: undecided ones give 2 or 4 candidate targets
    edge     0 <= q_x < w_j, 0 <= q_y < h_j: decided when every candidate agrees
    valid    d_j > depth_min and d_j < depth_max: stored fp32 numbers against fp32 thresholds, always decided
    disp     |fb / z - fb / d_j| < disp_thresh, per candidate
An undecided test exempts nothing.  Per (pixel, view) the outcome is ``certain`` (consistent, one known target), impossible, or
``und``ecided, which widens the pixel's count range [n_lo, n_hi] by one; the emit flag is decided when n_lo >= need or n_hi < need.
A view whose z interval reaches 0, or whose rounding interval spans more than two integers, is ``wild``: possibly consistent at an
unknown target.  Positions and colours are demanded wherever the pixel's consistent set is decided (n_lo == n_hi).

Colours are exact.  The channel sums are integers <= 64 * 255 = 16320 < 2^24 and (float)(n + 1) <= 64, both exact in fp32.  The fp32
quotient q is the correctly rounded s / (n + 1) < 256, so |q - s / (n + 1)| <= 2^-17.  s / (n + 1) is either a half-integer k + 1/2 --
an fp32 number, so q is exactly it and floorf(q + 0.5f) = k + 1 like the integer rule -- or at least 1 / (2 (n + 1)) >= 2^-7 away from
every half-integer; then q + 0.5f (one more rounding, <= 2^-17) stays on the same side of the integer, which itself is representable.
Hence floorf(q + 0.5f) = floor((2 s + n + 1) / (2 (n + 1))) in integers for every n + 1 <= 64 and s <= 255 (n + 1);
tests/test_fusion_ref_cpu.py verifies all of them."""
import numpy as np

EPS = 2.0 ** -24
TINY = 2.0 ** -149
F = np.float64
CRITERIA = ("front", "round", "edge", "disp")
UNDECIDED_CAP = 0.01
POS_SCALE = 1.0          # share of the analytic position bound that is demanded


def _f32exact(v):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(v, F).astype(np.float32).astype(F) == v


def _rnd(v, p):
    """bound after one fp32 rounding of a result within p of v (zero when the operands were exact and v is an fp32 number)"""
    r = p + (EPS * (np.abs(v) + p) + TINY)
    z = p == 0
    return np.where(z & _f32exact(v), 0.0, r) if z.any() else r


class IV:
    __slots__ = ("v", "e")

    def __init__(self, v, e=None):
        self.v = np.asarray(v, dtype=F)
        self.e = np.zeros_like(self.v) if e is None else np.asarray(e, dtype=F)


def _add(a, b):
    v = a.v + b.v
    return IV(v, _rnd(v, a.e + b.e))


def _sub(a, b):
    v = a.v - b.v
    return IV(v, _rnd(v, a.e + b.e))


def _mul(a, b):
    v = a.v * b.v
    return IV(v, _rnd(v, a.e * np.abs(b.v) + b.e * np.abs(a.v) + a.e * b.e))


def _mulc(m, x):
    v = m * x.v
    return IV(v, _rnd(v, np.abs(m) * x.e))


def _fma(m, x, acc):
    """fmaf(m, x, acc) with an exact factor m: one rounding"""
    v = m * x.v + acc.v
    return IV(v, _rnd(v, np.abs(m) * x.e + acc.e))


def _div(a, b):
    v = a.v / b.v
    den = np.abs(b.v) - b.e
    p = np.where((a.e == 0) & (b.e == 0), 0.0, np.where(den > 0, (a.e + np.abs(v) * b.e) / np.where(den > 0, den, 1.0), np.inf))
    pow2 = (b.e == 0) & (np.frexp(b.v)[0] == 0.5)
    return IV(v, np.where(pow2, p, _rnd(v, p)))


def _sqrt(s):
    v = np.sqrt(s.v)
    p = np.where(s.e == 0, 0.0, np.where(v > 0, s.e / np.where(v > 0, v, 1.0), np.sqrt(s.e)))
    return IV(v, _rnd(v, p))


def _sel(m, a, b):
    return IV(np.where(m, a.v, b.v), np.where(m, a.e, b.e))


def _mat(M, x, y, z):
    return tuple(_fma(M[3 * r + 2], z, _fma(M[3 * r + 1], y, _mulc(M[3 * r], x))) for r in range(3))


def _matT(M, x, y, z):
    return tuple(_fma(M[6 + c], z, _fma(M[3 + c], y, _mulc(M[c], x))) for c in range(3))


def _unproject(cam, x, y, d):
    """cam_unproject: R^T (d K^-1 (x, y, 1) - t)"""
    a = _mat(cam[9:18], _mul(x, d), _mul(y, d), d)
    return _matT(cam[18:27], *(_sub(a[k], IV(cam[27 + k])) for k in range(3)))


def _point(cam, X, Y, Z):
    """cam_point: K (R X + t), not divided"""
    c = _mat(cam[18:27], X, Y, Z)
    return _mat(cam[0:9], *(_add(c[k], IV(cam[27 + k])) for k in range(3)))


def _baseline(ci, cj):
    """fb_lds[j] = K_i[0] sqrtf(|R_i^T t_i - R_j^T t_j|^2)"""
    pi = _matT(ci[18:27], IV(ci[27]), IV(ci[28]), IV(ci[29]))
    pj = _matT(cj[18:27], IV(cj[27]), IV(cj[28]), IV(cj[29]))
    dx, dy, dz = (_sub(pi[k], pj[k]) for k in range(3))
    return _mulc(ci[0], _sqrt(_add(_add(_mul(dx, dx), _mul(dy, dy)), _mul(dz, dz))))


def thresholds(disp_thresh, depth_min=1e-3, depth_max=1e5):
    """the three thresholds as the kernel holds them: fp32 numbers"""
    return float(np.float32(disp_thresh)), float(np.float32(depth_min)), float(np.float32(depth_max))


def pad_views(depths, colors=None):
    """N maps of different sizes -> [N,H,W] float64 of their fp32 values (NaN outside), int64 colours [N,H,W,3], heights, widths"""
    N = len(depths)
    hs = np.array([d.shape[0] for d in depths])
    ws = np.array([d.shape[1] for d in depths])
    D = np.full((N, hs.max(), ws.max()), np.nan)
    C = np.zeros((N, hs.max(), ws.max(), 3), dtype=np.int64)
    for v, d in enumerate(depths):
        D[v, :hs[v], :ws[v]] = np.asarray(d, dtype=np.float32).astype(F)
        if colors is not None:
            C[v, :hs[v], :ws[v]] = np.asarray(colors[v])[..., :3]
    return D, C, hs, ws


def ref_pass(i, depths, colors, cams, used_i, disp_thresh, depth_min=1e-3, depth_max=1e5, debug=False):
    """Pass i for its active pixels (valid depth, used byte 0) -> dict of maps over view i ([J,h,w] per other view, J = N - 1, in
    view order ``js``); ``decide`` applies ``num_consistent``.  ``debug`` keeps the intermediate quantities of the active pixels
    (``dbg``, arrays [P] and [J,P] in row-major pixel order) for the exactness tests."""
    with np.errstate(all="ignore"):
        return _ref_pass(i, depths, colors, cams, used_i, *thresholds(disp_thresh, depth_min, depth_max), debug)


def _ref_pass(i, depths, colors, cams, used_i, thr, dmin, dmax, debug):
    cams = np.asarray(cams, dtype=np.float32).astype(F)
    N = len(depths)
    D, C, hs, ws = pad_views(depths, colors)
    h, w = int(hs[i]), int(ws[i])
    fvalid = lambda d: (d > dmin) & (d < dmax)
    d = D[i, :h, :w]
    active = fvalid(d) & (np.asarray(used_i) == 0)
    idx = np.flatnonzero(active.reshape(-1))
    P = len(idx)
    X = _unproject(cams[i], IV((idx % w).astype(F)), IV((idx // w).astype(F)), IV(d.reshape(-1)[idx]))
    js = np.array([j for j in range(N) if j != i])
    J = len(js)
    cj = cams[js].T[:, :, None]                                        # cj[k]: [J,1]
    hj, wj, jj = hs[js][:, None], ws[js][:, None], js[:, None]
    fb = _baseline(cams[i], cj)
    a, b, z = _point(cj, *X)
    front_t, front_f = z.v - z.e > 0, z.v + z.e <= 0
    half = IV(0.5)
    uh, vh = _add(_div(a, z), half), _add(_div(b, z), half)
    xl, xh, yl, yh = np.floor(uh.v - uh.e), np.floor(uh.v + uh.e), np.floor(vh.v - vh.e), np.floor(vh.v + vh.e)
    wild = ~front_f & (~front_t | ~(xh - xl <= 1) | ~(yh - yl <= 1))
    single = (xh == xl) & (yh == yl)
    fbz = _div(fb, z)
    live_any = ~front_f & ~wild
    cands = []
    for c in range(4):
        qx, qy = (xh if c & 1 else xl), (yh if c & 2 else yl)
        live = live_any & ((xh != xl) if c & 1 else True) & ((yh != yl) if c & 2 else True)
        if c and not live.any():
            continue
        inside = live & (qx >= 0) & (qx < wj) & (qy >= 0) & (qy < hj)
        qxi, qyi = np.where(inside, qx, 0).astype(np.int64), np.where(inside, qy, 0).astype(np.int64)
        dj = D[jj, qyi, qxi]
        ok = inside & fvalid(dj)
        djs = np.where(ok, dj, 1.0)
        disp = _sub(fbz, _div(fb, IV(djs)))
        av = np.abs(disp.v)
        cons_t, cons_f = ok & (av + disp.e < thr), ok & (av - disp.e >= thr)
        if c == 0:
            disp0 = disp
        cands.append({"live": live, "inside": inside, "ok": ok, "cons_t": cons_t, "cons_f": cons_f, "possible": ok & ~cons_f,
                      "qx": qxi, "qy": qyi, "dj": djs})
    c0 = cands[0]
    certain = live_any & front_t & single & c0["cons_t"]
    und = ~front_f & ~certain & (wild | np.any([c["possible"] for c in cands], axis=0))
    n_in = sum(c["inside"].astype(int) for c in cands)
    n_live = sum(c["live"].astype(int) for c in cands)
    undecided = {"front": int((~front_f & ~front_t).sum()),
                 "round": int((front_t & ~single).sum()),
                 "edge": int((live_any & (n_in > 0) & (n_in < n_live)).sum()),
                 "disp": int(np.any([c["ok"] & ~c["cons_t"] & ~c["cons_f"] for c in cands], axis=0).sum())}
    # the mean of the decided consistent set, in view order
    Xj = _unproject(cj, IV(c0["qx"].astype(F)), IV(c0["qy"].astype(F)), IV(c0["dj"]))
    zero = IV(np.zeros(P))
    S = [zero, zero, zero]
    n = np.zeros(P, dtype=np.int64)
    csum = C[i, :h, :w].reshape(-1, 3)[idx].copy()
    for k in range(J):
        m = certain[k]
        if not m.any():
            continue
        for ax in range(3):
            xk = IV(Xj[ax].v[k], Xj[ax].e[k])
            S[ax] = _sel(m, _sel(n == 0, xk, _add(S[ax], xk)), S[ax])
        csum += np.where(m[:, None], C[js[k], c0["qy"][k], c0["qx"][k]], 0)
        n += m
    inv = IV((n + 1).astype(F))
    out = [_sel(n == 0, X[ax], _div(_add(X[ax], S[ax]), inv)) for ax in range(3)]
    rgb = (2 * csum + (n + 1)[:, None]) // (2 * (n + 1)[:, None])

    def maps(arr, fill=0):
        """[..., P] -> [..., h, w]"""
        arr = np.asarray(arr)
        full = np.full(arr.shape[:-1] + (h * w,), fill, dtype=arr.dtype)
        full[..., idx] = arr
        return full.reshape(arr.shape[:-1] + (h, w))

    return {"i": i, "js": js, "active": active, "idx": idx, "certain": maps(certain), "und": maps(und), "wild": maps(wild),
            "cands": [{"possible": maps(c["possible"]), "qx": maps(c["qx"]), "qy": maps(c["qy"])} for c in cands],
            "hs": hs, "ws": ws, "xyz": np.stack([maps(o.v) for o in out], axis=-1), "bound": np.stack([maps(o.e) for o in out], axis=-1),
            "rgb": np.stack([maps(rgb[:, k]) for k in range(3)], axis=-1), "n_lo": maps(n), "n_hi": maps(n + und.sum(axis=0)),
            "undecided": undecided, "tuples": 4 * P * J,
            "dbg": {"X": X, "a": a, "b": b, "z": z, "uh": uh, "vh": vh, "fb": fb, "disp": disp0, "Xj": Xj, "out": out, "n": n,
                    "front_t": front_t, "front_f": front_f, "c0": c0, "certain": certain} if debug else None}


def decide(ref, need):
    """The pass's outcome under ``num_consistent``: emit flags (decided true / decided false), the pixels whose consistent set is
    decided, and per other view the marks that must and that may appear."""
    active = ref["active"]
    emit_t = active & (ref["n_lo"] >= need)
    emit_f = ~active | (ref["n_hi"] < need)
    maybe = active & (ref["n_hi"] >= need)
    c0 = ref["cands"][0]
    must, may = {}, {}
    for k, j in enumerate(ref["js"]):
        mu = np.zeros((ref["hs"][j], ref["ws"][j]), dtype=bool)
        m = emit_t & ref["certain"][k]
        mu[c0["qy"][k][m], c0["qx"][k][m]] = True
        ma = mu.copy()
        if (maybe & ref["wild"][k]).any():
            ma[:] = True
        else:
            for c in ref["cands"]:
                m = maybe & c["possible"][k] & (ref["certain"][k] | ref["und"][k])
                ma[c["qy"][k][m], c["qx"][k][m]] = True
        must[int(j)], may[int(j)] = mu, ma
    return {"active": active, "emit_t": emit_t, "emit_f": emit_f, "set_decided": active & (ref["n_lo"] == ref["n_hi"]),
            "must": must, "may": may}


def compare(ref, dec, got, before, after, label=""):
    """A pass's outputs ``got`` = (xyz [M,3] fp32, rgb [M,3] uint8, pix [M]) and the masks before / after it against the reference
    -> (list of violations, stats).  Nothing is exempt: every decided emit flag, every decided set's position (within its own
    propagated bound) and colour (exactly), every mark."""
    xyz, rgb, pix = (np.asarray(g) for g in got)
    i = ref["i"]
    h, w = ref["active"].shape
    bad, st = [], {"points": int(len(pix)), "pos_ratio": 0.0, "pos_checked": 0, "old_bar": 0.0, "bound_rel": 0.0, "n_emit": 0,
                   "n_pos": 0, "n_rgb": 0, "n_stray": 0, "n_missing": 0, "n_other": 0}
    pix = pix.astype(np.int64)
    if len(pix) and (pix.min() < 0 or pix.max() >= h * w or not (np.diff(pix) > 0).all()):
        bad.append(f"{label}: pixel indices not strictly increasing inside [0, {h * w})")
        st["n_other"] += 1
        return bad, st
    if not (xyz.shape == (len(pix), 3) and rgb.shape == (len(pix), 3)):
        bad.append(f"{label}: output shapes {xyz.shape} {rgb.shape} for {len(pix)} points")
        st["n_other"] += 1
        return bad, st
    emit = np.zeros(h * w, dtype=bool)
    emit[pix] = True
    emit = emit.reshape(h, w)
    k = int((emit & dec["emit_f"]).sum())
    if k:
        bad.append(f"{label}: {k} pixels emitted that decidedly must not")
        st["n_emit"] += k
    k = int((~emit & dec["emit_t"]).sum())
    if k:
        bad.append(f"{label}: {k} pixels not emitted that decidedly must")
        st["n_emit"] += k
    sel = dec["set_decided"].reshape(-1)[pix]
    if sel.any():
        want = ref["xyz"].reshape(-1, 3)[pix[sel]]
        bound = ref["bound"].reshape(-1, 3)[pix[sel]] * POS_SCALE
        with np.errstate(invalid="ignore", divide="ignore"):
            err = np.abs(xyz[sel].astype(F) - want)
            ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))
        ratio = np.where(np.isnan(ratio), np.inf, ratio)
        st["pos_ratio"], st["pos_checked"] = float(ratio.max()), int(sel.sum())
        scale = np.maximum(np.abs(want).max(axis=1), 1e-6)
        st["old_bar"] = float((err.max(axis=1) / scale).max())
        st["bound_rel"] = float((bound.max(axis=1) / scale).max())
        if not (ratio <= 1.0).all():
            st["n_pos"] += int((ratio > 1.0).any(axis=1).sum())
            bad.append(f"{label}: {int((ratio > 1.0).any(axis=1).sum())} positions outside their bound (worst {ratio.max():.3g} of it)")
        if not st["old_bar"] < 1e-5:
            bad.append(f"{label}: position rel err {st['old_bar']:.2e}")
        k = int((rgb[sel].astype(np.int64) != ref["rgb"].reshape(-1, 3)[pix[sel]]).any(axis=1).sum())
        if k:
            bad.append(f"{label}: {k} colours differ from the integer rule")
            st["n_rgb"] += k
    if not np.array_equal(after[i], before[i]):
        bad.append(f"{label}: the pass changed used_{i}")
        st["n_other"] += 1
    for j in dec["must"]:
        b, a = np.asarray(before[j]), np.asarray(after[j])
        k = int(((b != 0) & (a == 0)).sum() + ((a != b) & (a != 1)).sum())
        if k:
            bad.append(f"{label}: view {j}: {k} marks removed or set to something other than 1")
            st["n_other"] += k
        new = (a != 0) & (b == 0)
        k = int((new & ~dec["may"][j]).sum())
        if k:
            bad.append(f"{label}: view {j}: {k} new marks outside every candidate target of a possibly emitting pixel")
            st["n_stray"] += k
        k = int((dec["must"][j] & (a == 0)).sum())
        if k:
            bad.append(f"{label}: view {j} lacks {k} marks of decided points")
            st["n_missing"] += k
    return bad, st


def run_case(case, step, *, name=None, passes=None, on_pass=None):
    """Every pass of ``case`` (tests/_fusion_cases.py) in order: ``step(i, used)`` runs pass i on copies of the masks ``used`` (numpy)
    and returns (xyz, rgb, pix, masks after).  Each pass is compared on its own, with the masks the implementation itself left
    before it, so an undecided outcome of an earlier pass cannot cascade.  -> (violations, stats per pass, undecided tuples, tuples)"""
    N = len(case["depths"])
    used = [u.copy() for u in case["used0"]]
    thr, need = case["disp_thresh"], case["num_consistent"]
    bad, stats, und, tup = [], [], {c: 0 for c in CRITERIA}, 0
    for i in (range(N) if passes is None else passes):
        ref = ref_pass(i, case["depths"], case["colors"], case["cams"], used[i], thr)
        dec = decide(ref, need)
        xyz, rgb, pix, after = step(i, [u.copy() for u in used])
        b, st = compare(ref, dec, (xyz, rgb, pix), used, after, label=f"{name} pass {i}")
        if on_pass is not None:
            on_pass(i, ref, dec, (xyz, rgb, pix), used, after)
        bad += b
        st["decided_sets"] = int(dec["set_decided"].sum())
        st["active"] = int(dec["active"].sum())
        stats.append(st)
        for c in CRITERIA:
            und[c] += ref["undecided"][c]
        tup += ref["tuples"]
        used = [np.asarray(a).copy() for a in after]
    return bad, stats, und, tup
