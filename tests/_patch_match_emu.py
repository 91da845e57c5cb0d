"""fp32 numpy emulation of csrc/patch_match.hip in the kernel's operation order: float32 at every step, the same association,
float64 window sums.  It stands in for the GPU where there is none (tests/test_patch_match_ref_cpu.py holds it to the bounds of
tests/_patch_match_bounds.py), and it takes planted errors (``plant``) that the bounds must catch:

  noclamp     bilinear without the edge clamp            nocolour   weights without the colour term
  cov         cov without - mr ms                        centre_rm  the centre at the reciprocal-multiply position        
  half_even   round-half-even in e_s                     nocap      e_s not capped
  mean_all    the mean over all sources, not the top_k   dist2      neighbour distance 2 instead of 3
  tie_high    ties go to the higher index                axis       the perturbation's tangent axis switched at |nx| < 0.9
  cos1        the filter's 3 deg test done with cos 1 deg
"""
from __future__ import annotations

import numpy as np

from tests import _patch_match_bounds as PB
from tests import _patch_match_ref as PR
from tests._fusion_ref import cam_rows

f = np.float32
PLANTS = ("noclamp", "nocolour", "cov", "centre_rm", "half_even", "nocap", "mean_all", "dist2", "tie_high", "axis", "cos1")
COS1, COS3 = f(0.99984769515639123916), f(0.99862953475457387378)


def _a(x):
    return np.asarray(x, dtype=f)


def _bil(img, u, v, plant=None):
    h, w = img.shape
    if plant != "noclamp":
        u = np.fmin(np.fmax(u, f(0)), f(w - 1))
        v = np.fmin(np.fmax(v, f(0)), f(h - 1))
    else:
        u, v = np.nan_to_num(u, nan=0.0, posinf=1e6, neginf=-1e6).astype(f), np.nan_to_num(v, nan=0.0, posinf=1e6, neginf=-1e6).astype(f)
    x0 = np.clip(np.clip(u, -1e6, 1e6).astype(np.int64), 0, w - 1)
    y0 = np.clip(np.clip(v, -1e6, 1e6).astype(np.int64), 0, h - 1)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    fx, fy = u - x0.astype(f), v - y0.astype(f)
    top = (f(1) - fx) * img[y0, x0] + fx * img[y0, x1]
    bot = (f(1) - fx) * img[y1, x0] + fx * img[y1, x1]
    return (f(1) - fy) * top + fy * bot


def _window(ref, rows, cols, radius, step, plant):
    h, w = ref.shape
    oy, ox = PR.offsets(radius, step)
    rr = np.clip(rows[:, None] + oy[None], 0, h - 1)
    cc = np.clip(cols[:, None] + ox[None], 0, w - 1)
    rp = ref[rr, cc] - ref[rows, cols][:, None]
    inv2ss = f(1) / (f(2) * f(radius) * f(radius))
    inv2sc = f(1) / (f(2) * f(PR.SIGMA_COLOR) * f(PR.SIGMA_COLOR))
    arg = -_a((oy ** 2 + ox ** 2)[None]) * inv2ss - (f(0) if plant == "nocolour" else rp * rp * inv2sc)
    wgt = np.exp(arg.astype(f)).astype(f)
    wr = (wgt * rp).astype(f)
    W = wgt.astype(np.float64).sum(1)
    inv_w = 1.0 / W
    mr = wr.astype(np.float64).sum(1) * inv_w
    vr = (wr.astype(np.float64) * rp.astype(np.float64)).sum(1) * inv_w - mr * mr
    return dict(wgt=wgt, wr=wr, rp=rp, inv_w=inv_w, mr=mr, vr=vr, oy=oy, ox=ox)


def _geom(G, s, sdepth, d, col, row, plant):
    g = [x[s] for x in G]
    with np.errstate(all="ignore"):
        y = [d * (g[3 * i] * col + g[3 * i + 1] * row + g[3 * i + 2]) + g[9 + i] for i in range(3)]
        ok = y[2] > 0
        u, v = y[0] / y[2], y[1] / y[2]
        ok &= (np.abs(u) < f(2 ** 30)) & (np.abs(v) < f(2 ** 30))
        u, v = np.where(ok, u, f(0)), np.where(ok, v, f(0))
        if plant == "half_even":
            qx, qy = np.rint(u).astype(np.int64), np.rint(v).astype(np.int64)
        else:
            rnd = lambda x: (np.trunc(x) + np.sign(x) * (np.abs(x - np.trunc(x)) >= f(0.5))).astype(np.int64)
            qx, qy = rnd(u), rnd(v)
        hs, ws = sdepth.shape
        ok &= (qx >= 0) & (qx < ws) & (qy >= 0) & (qy < hs)
        ds = np.where(ok, sdepth[np.clip(qy, 0, hs - 1), np.clip(qx, 0, ws - 1)], f(0))
        ok &= ds > 0
        fx, fy = qx.astype(f), qy.astype(f)
        r = [ds * (g[15 + 3 * i] * fx + g[16 + 3 * i] * fy + g[17 + 3 * i]) + g[24 + i] for i in range(3)]
        ok &= r[2] > 0
        ex, ey = r[0] / r[2] - col, r[1] / r[2] - row
        err = np.sqrt(ex * ex + ey * ey)
        if plant != "nocap":
            err = np.fmin(err, f(PR.GEOM_EMAX))
    return np.where(ok, err, f(PR.GEOM_EMAX)).astype(f)


def evaluate(ref, srcs, cams, rows, cols, hyp, radius=5, step=1, top_k=None, src_depths=None, plant=None, window=None):
    """pm_eval at the pixels (rows, cols) for the hypotheses hyp [N,4] fp32 -> (c [S,N], e [S,N] or None, agg [N], passes [N]: the
    filter's count) as fp32."""
    ref = _a(ref)
    S, N = len(srcs), len(rows)
    top_k = min(S, 3) if top_k is None else top_k
    G = PB.source_blocks(cams, wrap=_a)
    kinv = [f(x) for x in cam_rows(cams)[0, 9:18]]
    win = _window(ref, rows, cols, radius, step, plant) if window is None else window
    col, row = _a(cols), _a(rows)
    hyp = _a(hyp)
    d, nx, ny, nz = hyp[:, 0], hyp[:, 1], hyp[:, 2], hyp[:, 3]
    c_out, e_out = np.full((S, N), f(2)), np.zeros((S, N), f)
    npass = np.zeros(N, np.int64)
    with np.errstate(all="ignore"):
        m = [kinv[3 * i] * col + kinv[3 * i + 1] * row + kinv[3 * i + 2] for i in range(3)]
        rho = d * (nx * m[0] + ny * m[1] + nz * m[2])
        ir = f(1) / rho
        g = [(kinv[i] * nx + kinv[3 + i] * ny + kinv[6 + i] * nz) * ir for i in range(3)]
        X = [d * m[i] for i in range(3)]
        nX = np.sqrt(X[0] * X[0] + X[1] * X[1] + X[2] * X[2])
        qx, qy = _a(cols[:, None] + win["ox"][None]), _a(rows[:, None] + win["oy"][None])
        wd, wrd = win["wgt"].astype(np.float64), win["wr"].astype(np.float64)
        for s in range(S):
            img = _a(srcs[s])
            hs, ws = img.shape
            gs = [x[s] for x in G]
            H = [gs[3 * i + j] + gs[9 + i] * g[j] for i in range(3) for j in range(3)]
            xc = [H[3 * i] * col + H[3 * i + 1] * row + H[3 * i + 2] for i in range(3)]
            pos = xc[2] > 0
            u, v = np.where(pos, xc[0] / xc[2], f(0)), np.where(pos, xc[1] / xc[2], f(0))
            if plant == "centre_rm":                           # one (u, v) for the inside test and the sample, as the taps get theirs
                izc = f(1) / xc[2]
                u, v = np.where(pos, xc[0] * izc, f(0)), np.where(pos, xc[1] * izc, f(0))
            centre_ok = pos & (u >= 0) & (u <= f(ws - 1)) & (v >= 0) & (v <= f(hs - 1))
            r = [X[i] - gs[12 + i] for i in range(3)]
            cosa = (X[0] * r[0] + X[1] * r[1] + X[2] * r[2]) / (nX * np.sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]))
            ok = centre_ok & (win["vr"] >= np.float64(f(PR.MIN_VAR))) & (cosa <= COS1)
            sc = _bil(img, u, v, plant)
            Ht = [x[:, None] for x in H]
            x = [Ht[3 * i] * qx + Ht[3 * i + 1] * qy + Ht[3 * i + 2] for i in range(3)]
            iz = f(1) / x[2]
            ut, vt = np.where(x[2] > 0, x[0] * iz, f(0)), np.where(x[2] > 0, x[1] * iz, f(0))
            val = (_bil(img, ut, vt, plant) - sc[:, None]).astype(f).astype(np.float64)
            wv = wd * val
            ms = wv.sum(1) * win["inv_w"]
            vs = (wv * val).sum(1) * win["inv_w"] - ms * ms
            cov = (wrd * val).sum(1) * win["inv_w"] - (0.0 if plant == "cov" else win["mr"] * ms)
            ncc = (cov / np.sqrt(win["vr"] * vs)).astype(f)
            c = np.fmin(np.fmax(f(1) - ncc, f(0)), f(2))
            c = np.where(ok & (vs >= np.float64(f(PR.MIN_VAR))), c, f(2)).astype(f)
            c_out[s] = c
            e = np.zeros(N, f)
            if src_depths is not None:
                e = _geom(G, s, _a(src_depths[s]), d, col, row, plant)
                e_out[s] = e
            npass += (c <= f(PR.FILTER_MAX_COST)) & (cosa <= (COS1 if plant == "cos1" else COS3)) & (e <= f(PR.FILTER_MAX_ERR))
        cc = c_out if src_depths is None else (c_out + f(PR.GEOM_LAMBDA) * np.fmin(e_out, f(PR.GEOM_EMAX))).astype(f)
        k = S if plant == "mean_all" else top_k
        srt = np.sort(cc, axis=0)[:k]
        acc = np.zeros(N, f)
        for i in range(k):
            acc = (acc + srt[i]).astype(f)
        agg = (acc / f(k)).astype(f)
    return c_out, (e_out if src_depths is not None else None), agg, npass


def _m(cams, rows, cols):
    kinv = [f(x) for x in cam_rows(cams)[0, 9:18]]
    col, row = _a(cols), _a(rows)
    return kinv, [kinv[3 * i] * col + kinv[3 * i + 1] * row + kinv[3 * i + 2] for i in range(3)]


def _uni(seed, view, pix, iteration, colour, slot):
    return PR.pm_uniform(seed, view, pix, iteration, colour, slot).astype(f)


def random_hyp(cams, rows, cols, w, dmin, dmax, seed, view, iteration, colour):
    _, m = _m(cams, rows, cols)
    pix = rows.astype(np.int64) * w + cols
    ud, uz, ua = (_uni(seed, view, pix, iteration, colour, s) for s in (PR.SLOT_RDEPTH, PR.SLOT_RZ, PR.SLOT_RAZ))
    lo, hi = f(1) / f(dmax), f(1) / f(dmin)
    d = f(1) / (lo + ud * (hi - lo))
    z = f(1) - f(2) * uz
    r = np.sqrt(np.fmax(f(0), f(1) - z * z))
    al = f(6.283185307179586) * ua
    n = np.stack([r * np.cos(al), r * np.sin(al), z], -1).astype(f)
    flip = n[:, 0] * m[0] + n[:, 1] * m[1] + n[:, 2] * m[2] > 0
    n = np.where(flip[:, None], -n, n)
    return np.concatenate([d[:, None], n], 1).astype(f)


def perturb_hyp(cams, rows, cols, w, cur, dmin, dmax, delta, theta, seed, view, iteration, colour, plant=None):
    _, m = _m(cams, rows, cols)
    pix = rows.astype(np.int64) * w + cols
    up, ua, ud = (_uni(seed, view, pix, iteration, colour, s) for s in (PR.SLOT_PHI, PR.SLOT_ALPHA, PR.SLOT_DEPTH))
    nx, ny, nz = cur[:, 1], cur[:, 2], cur[:, 3]
    ax = np.abs(nx) < f(0.9)
    if plant == "axis":
        ax = ~ax
    z = np.zeros_like(nx)
    with np.errstate(all="ignore"):
        e1 = [np.where(ax, z, -nz), np.where(ax, nz, z), np.where(ax, -ny, nx)]
        il = f(1) / np.sqrt(e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2])
        e1 = [x * il for x in e1]
        e2 = [ny * e1[2] - nz * e1[1], nz * e1[0] - nx * e1[2], nx * e1[1] - ny * e1[0]]
        phi, al = f(theta) * up, f(6.283185307179586) * ua
        ca, sa, cp, sp = np.cos(al), np.sin(al), np.cos(phi), np.sin(phi)
        p = [cp * c + sp * (ca * a + sa * b) for c, a, b in zip((nx, ny, nz), e1, e2)]
        ip = f(1) / np.sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2])
        p = [x * ip for x in p]
        face = p[0] * m[0] + p[1] * m[1] + p[2] * m[2] < 0
        p = [np.where(face, a, b) for a, b in zip(p, (nx, ny, nz))]
        lo, hi = f(1) / f(dmax), f(1) / f(dmin)
        inv = np.fmin(np.fmax(f(1) / cur[:, 0] + (f(2) * ud - f(1)) * f(delta) * (hi - lo), lo), hi)
        return np.stack([f(1) / inv] + p, -1).astype(f)


def half_step(state, ref, srcs, cams, dmin, dmax, *, colour, iteration, delta, theta, seed, view, src_depths=None, radius=5, step=1,
              top_k=None, plant=None):
    """-> (new state fp32 [h,w,4], choice [N], candidates fp32 [N,11,4] (0 where skipped)) for the colour's pixels in row-major
    order (PR.colour_pixels)."""
    state = _a(state)
    h, w, _ = state.shape
    rows, cols = PR.colour_pixels(h, w, colour)
    N = len(rows)
    kinv, m = _m(cams, rows, cols)
    cand = np.zeros((N, PR.NUM_CAND, 4), f)
    live = np.ones((N, PR.NUM_CAND), bool)
    cur = state[rows, cols]
    cand[:, 0] = cur
    nb = PR.NEIGHBOURS if plant != "dist2" else tuple((a // 3 * 2 if abs(a) == 3 else a, b // 3 * 2 if abs(b) == 3 else b)
                                                      for a, b in PR.NEIGHBOURS)
    with np.errstate(all="ignore"):
        for k, (dr, dc) in enumerate(nb, start=1):
            qr, qc = rows + int(dr), cols + int(dc)
            inside = (qr >= 0) & (qr < h) & (qc >= 0) & (qc < w)
            q = state[np.clip(qr, 0, h - 1), np.clip(qc, 0, w - 1)]
            fq, fr = _a(qc), _a(qr)
            Q = [q[:, 0] * (kinv[3 * i] * fq + kinv[3 * i + 1] * fr + kinv[3 * i + 2]) for i in range(3)]
            d = (q[:, 1] * Q[0] + q[:, 2] * Q[1] + q[:, 3] * Q[2]) / (q[:, 1] * m[0] + q[:, 2] * m[1] + q[:, 3] * m[2])
            lv = inside & (d >= f(dmin)) & (d <= f(dmax))
            live[:, k] = lv
            cand[:, k] = np.where(lv[:, None], np.concatenate([d[:, None], q[:, 1:]], 1), f(0))
    cand[:, 9] = perturb_hyp(cams, rows, cols, w, cur, dmin, dmax, delta, theta, seed, view, iteration, colour, plant)
    cand[:, 10] = random_hyp(cams, rows, cols, w, dmin, dmax, seed, view, iteration, colour)
    win = _window(_a(ref), rows, cols, radius, step, plant)
    best_c, best_k = np.zeros(N, f), np.zeros(N, np.int64)
    for k in range(PR.NUM_CAND):
        idx = np.nonzero(live[:, k])[0]
        if not len(idx):
            continue
        w_k = {key: (val[idx] if key not in ("oy", "ox") else val) for key, val in win.items()}
        _, _, agg, _ = evaluate(ref, srcs, cams, rows[idx], cols[idx], cand[idx, k], radius, step, top_k, src_depths, plant, w_k)
        better = (agg <= best_c[idx]) if plant == "tie_high" else (agg < best_c[idx])
        if k == 0:
            better = np.ones(len(idx), bool)
        best_c[idx] = np.where(better, agg, best_c[idx])
        best_k[idx] = np.where(better, k, best_k[idx])
    new = state.copy()
    new[rows, cols] = cand[np.arange(N), best_k]
    return new, best_k, cand


def filter_state(state, ref, srcs, cams, src_depths, radius=5, step=1, plant=None):
    state = _a(state)
    h, w, _ = state.shape
    rows, cols = np.divmod(np.arange(h * w), w)
    st = state.reshape(-1, 4)
    live = st[:, 0] > 0
    hyp = np.where(live[:, None], st, _a([1.0, 0.0, 0.0, -1.0])[None])
    _, _, _, npass = evaluate(ref, srcs, cams, rows, cols, hyp, radius, step, 1, src_depths, plant)
    count = np.where(live, npass, 0)
    keep = count >= PR.FILTER_MIN_CONSISTENT
    return np.where(keep, st[:, 0], f(0)).reshape(h, w), np.where(keep[:, None], st[:, 1:], f(0)).reshape(h, w, 3), count.reshape(h, w)
