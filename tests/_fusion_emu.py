"""numpy float32 emulation of one pass of the depth-map fusion kernel (csrc/depth_fusion.hip) in the kernel's own order: every
product, sum, quotient and square root rounded to fp32, ``fmaf`` as a float64 multiply-add rounded to fp32 (the product of two fp32
numbers is exact in float64), the views in index order, the mean divided by (float)(n + 1).  ``plant`` swaps in one deliberate error
(``PLANTS``); tests/test_fusion_ref_cpu.py shows that the float64 reference with its bounds (tests/_fusion_bounds.py) accepts the
emulation and rejects every plant."""
import numpy as np

f32 = np.float32
F = np.float64
PLANTS = ("half_even", "trunc", "disp_le", "valid_ge", "f_j", "t_baseline", "no_front", "unrounded_neighbour", "div_n",
          "colour_trunc", "need_gt", "marks_nonemit", "skip_used", "double_thresholds")


def _fma(a, b, c):
    return (np.asarray(a, F) * np.asarray(b, F) + np.asarray(c, F)).astype(f32)


def _mat(M, x, y, z):
    return tuple(_fma(M[3 * r + 2], z, _fma(M[3 * r + 1], y, M[3 * r] * x)) for r in range(3))


def _matT(M, x, y, z):
    return tuple(_fma(M[6 + c], z, _fma(M[3 + c], y, M[c] * x)) for c in range(3))


def _unproject(cam, x, y, d):
    a = _mat(cam[9:18], x * d, y * d, d)
    return _matT(cam[18:27], a[0] - cam[27], a[1] - cam[28], a[2] - cam[29])


def _point(cam, X, Y, Z):
    c = _mat(cam[18:27], X, Y, Z)
    return _mat(cam[0:9], c[0] + cam[27], c[1] + cam[28], c[2] + cam[29])


def emu_pass(i, depths, colors, cams, used, *, disp_thresh, num_consistent, depth_min=1e-3, depth_max=1e5, plant=None):
    """depths N x fp32 [h,w], colors N x uint8 [h,w,3], cams fp32 [N,30], used N x uint8 (NOT modified) ->
    (xyz fp32 [M,3], rgb uint8 [M,3], pix int64 [M] row-major, the masks after the pass)."""
    assert plant is None or plant in PLANTS
    with np.errstate(all="ignore"):
        return _emu_pass(i, depths, colors, np.asarray(cams, dtype=f32), used, disp_thresh, num_consistent, depth_min, depth_max, plant)


def _emu_pass(i, depths, colors, cams, used, thr, need, dmin, dmax, plant):
    N = len(depths)
    if plant != "double_thresholds":
        thr, dmin, dmax = f32(thr), f32(dmin), f32(dmax)
    thr, dmin, dmax = F(thr), F(dmin), F(dmax)          # (compared as float64 numbers: exact for fp32 values either way)
    if plant == "valid_ge":
        fvalid = lambda d: (d.astype(F) >= dmin) & (d.astype(F) <= dmax)
    else:
        fvalid = lambda d: (d.astype(F) > dmin) & (d.astype(F) < dmax)
    d = np.asarray(depths[i], dtype=f32)
    h, w = d.shape
    active = fvalid(d) & (np.asarray(used[i]) == 0)
    ys, xs = np.meshgrid(np.arange(h, dtype=f32), np.arange(w, dtype=f32), indexing="ij")
    ci = cams[i]
    X, Y, Z = _unproject(ci, xs, ys, np.where(active, d, f32(1)))
    pi = _matT(ci[18:27], ci[27], ci[28], ci[29])
    sx, sy, sz = (np.zeros((h, w), f32) for _ in range(3))
    csum = np.zeros((h, w, 3), dtype=np.int64)
    n = np.zeros((h, w), dtype=np.int64)
    hits = []
    for j in range(N):
        if j == i:
            continue
        cj = cams[j]
        dj_map = np.asarray(depths[j], dtype=f32)
        hj, wj = dj_map.shape
        pj = _matT(cj[18:27], cj[27], cj[28], cj[29])
        if plant == "t_baseline":
            dx, dy, dz = ci[27] - cj[27], ci[28] - cj[28], ci[29] - cj[29]
        else:
            dx, dy, dz = pi[0] - pj[0], pi[1] - pj[1], pi[2] - pj[2]
        fb = (cj[0] if plant == "f_j" else ci[0]) * np.sqrt(dx * dx + dy * dy + dz * dz)
        a, b, z = _point(cj, X, Y, Z)
        front = np.ones((h, w), bool) if plant == "no_front" else z > 0
        u, v = a / z, b / z
        if plant == "half_even":
            fx, fy = np.rint(u), np.rint(v)
        elif plant == "trunc":
            fx, fy = np.trunc(u), np.trunc(v)
        else:
            fx, fy = np.floor(u + f32(0.5)), np.floor(v + f32(0.5))
        inb = active & front & (fx >= 0) & (fx < f32(wj)) & (fy >= 0) & (fy < f32(hj))
        qx, qy = np.where(inb, fx, 0).astype(np.int64), np.where(inb, fy, 0).astype(np.int64)
        dj = dj_map[qy, qx]
        ok = inb & fvalid(dj)
        if plant == "skip_used":
            ok &= np.asarray(used[j])[qy, qx] == 0
        disp = np.abs(fb / z - fb / dj)
        cons = ok & ((disp.astype(F) <= thr) if plant == "disp_le" else (disp.astype(F) < thr))
        djs = np.where(cons, dj, f32(1))
        if plant == "unrounded_neighbour":
            Xj = _unproject(cj, u, v, djs)
        else:
            Xj = _unproject(cj, qx.astype(f32), qy.astype(f32), djs)
        sx, sy, sz = np.where(cons, sx + Xj[0], sx), np.where(cons, sy + Xj[1], sy), np.where(cons, sz + Xj[2], sz)
        csum += np.where(cons[..., None], np.asarray(colors[j])[qy, qx][..., :3].astype(np.int64), 0)
        n += cons
        hits.append((j, cons, qx, qy))
    emit = active & ((n > need) if plant == "need_gt" else (n >= need))
    inv = (n if plant == "div_n" else n + 1).astype(f32)
    xyz = np.stack(((X + sx) / inv, (Y + sy) / inv, (Z + sz) / inv), axis=-1).astype(f32)
    csum += np.asarray(colors[i])[..., :3].astype(np.int64)
    q = csum.astype(f32) / inv[..., None]
    rgb = (np.floor(q) if plant == "colour_trunc" else np.floor(q + f32(0.5)))
    after = [np.asarray(u_).copy() for u_ in used]
    for j, cons, qx, qy in hits:
        m = cons & (active if plant == "marks_nonemit" else emit)
        after[j][qy[m], qx[m]] = 1
    pix = np.flatnonzero(emit.reshape(-1))
    return xyz.reshape(-1, 3)[pix], np.clip(np.nan_to_num(rgb.reshape(-1, 3)[pix]), 0, 255).astype(np.uint8), pix, after
