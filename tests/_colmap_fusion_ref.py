"""numpy restatement of the COLMAP-style stereo fusion, the yardstick of csrc/colmap_fusion.hip, and
COLMAP's sequential StereoFusion loop as recalled there, for measuring how far the parallel rule deviates from it.

Geometry is float64 from the float32 inputs (depth maps, camera blocks [N,30] = K, K^-1, R, t), written in the kernel's operation
order with no fused multiply-adds, so the kernel's values are reproduced bit for bit.  ``parallel_pass`` also reports the smallest
relative distance of any decision it took to its threshold (``margin``); tests keep their scenes at least 1e-9 away."""
from __future__ import annotations

from collections import deque

import numpy as np

from tests._fusion_ref import cam_rows

PIX_LIMIT = float(1 << 30)
INV_SQRT3 = 0.57735026918962573
FLT_EPS = float(np.finfo(np.float32).eps)


def unproject(c, x, y, d):
    """R^T (d K^-1 (x, y, 1) - t) in the kernel's order; c one float64 camera row, x, y, d arrays -> (X, Y, Z)."""
    px, py, pz = x * d, y * d, d
    a0 = c[9] * px + c[10] * py + c[11] * pz
    a1 = c[12] * px + c[13] * py + c[14] * pz
    a2 = c[15] * px + c[16] * py + c[17] * pz
    b0, b1, b2 = a0 - c[27], a1 - c[28], a2 - c[29]
    return (c[18] * b0 + c[21] * b1 + c[24] * b2, c[19] * b0 + c[22] * b1 + c[25] * b2, c[20] * b0 + c[23] * b1 + c[26] * b2)


def project(c, X, Y, Z):
    """K (R X + t) -> (x, y, z)."""
    e0 = c[18] * X + c[19] * Y + c[20] * Z + c[27]
    e1 = c[21] * X + c[22] * Y + c[23] * Z + c[28]
    e2 = c[24] * X + c[25] * Y + c[26] * Z + c[29]
    return c[0] * e0 + c[1] * e1 + c[2] * e2, c[3] * e0 + c[4] * e1 + c[5] * e2, c[6] * e0 + c[7] * e1 + c[8] * e2


def round_away(v):
    """C ``round``: half away from zero (v - trunc(v) is exact)."""
    t = np.trunc(v)
    return t + np.where(np.abs(v - t) >= 0.5, np.sign(v), 0.0)


def view_normal(c):
    """R^T (1, 1, 1) / sqrt(3) rounded to float32."""
    return np.array([c[18] * INV_SQRT3 + c[21] * INV_SQRT3 + c[24] * INV_SQRT3, c[19] * INV_SQRT3 + c[22] * INV_SQRT3 + c[25] * INV_SQRT3,
                     c[20] * INV_SQRT3 + c[23] * INV_SQRT3 + c[26] * INV_SQRT3]).astype(np.float32)


def depth_ok(d):
    return (d > 0) & (d <= np.finfo(np.float32).max)


def find_next_image_order(overlap):
    """COLMAP's FindNextImage over all views: after view prev, the first view of overlap[prev] not yet processed, else the lowest
    unprocessed view."""
    n = len(overlap)
    done = [False] * n
    order, prev = [], -1
    for _ in range(n):
        nxt = next((m for m in overlap[prev] if not done[m]), None) if prev >= 0 else None
        if nxt is None:
            nxt = min(v for v in range(n) if not done[v])
        order.append(nxt)
        done[nxt] = True
        prev = nxt
    return order


def adjacency(overlap, n):
    a = np.zeros((n, n), dtype=bool)
    for k, lst in enumerate(overlap):
        for m in lst:
            if m != k:
                a[k, m] = True
    return a


def _fkey(v):
    u = np.asarray(v, dtype=np.float32).view(np.uint32)
    return np.where(u & 0x80000000, ~u, u | 0x80000000).astype(np.uint32)


def median_f32(v):
    """Median in the IEEE total order; an even count gives (a + b) * 0.5 in float32."""
    v = np.asarray(v, dtype=np.float32)
    s = v[np.argsort(_fkey(v), kind="stable")]
    n = len(s)
    if n % 2:
        return s[n // 2]
    return np.float32((s[n // 2 - 1] + s[n // 2]) * np.float32(0.5))


def median_u8(v):
    s = np.sort(np.asarray(v, dtype=np.int64))
    n = len(s)
    return int(s[n // 2]) if n % 2 else int((s[n // 2 - 1] + s[n // 2] + 1) >> 1)


def emit_point(xyz, normals, colors):
    """Cluster nodes -> (xyz fp32 [3], normal fp32 [3], rgb uint8 [3]) or None when the normal's median has norm < FLT_EPSILON."""
    med = np.array([median_f32(xyz[:, d]) for d in range(3)], dtype=np.float32)
    mn = np.array([median_f32(normals[:, d]) for d in range(3)], dtype=np.float32)
    g = mn.astype(np.float64)
    norm = np.sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2])
    if not norm >= FLT_EPS:
        return None
    rgb = np.array([median_u8(colors[:, d]) for d in range(3)], dtype=np.uint8)
    return med, (g / norm).astype(np.float32), rgb


class _Margin:
    def __init__(self):
        self.v = np.inf

    def rel(self, lhs, thr):
        if np.size(lhs):
            self.v = min(self.v, float(np.min(np.abs(lhs - thr))) / abs(thr))

    def rounding(self, u):
        if np.size(u):
            f = np.abs(u - np.trunc(u))
            self.v = min(self.v, float(np.min(np.abs(f - 0.5) / np.maximum(np.abs(u), 1.0))))


def _target(c, X, Y, Z, c0x, c0y, W, margin):
    """Window bit of round(P X) for the window at (c0x, c0y), -1 outside."""
    S = 2 * W + 1
    x, y, z = project(c, X, Y, Z)
    with np.errstate(divide="ignore", invalid="ignore"):
        u, v = x / z, y / z
    ok = (np.abs(u) < PIX_LIMIT) & (np.abs(v) < PIX_LIMIT)
    margin.rounding(u[ok])
    margin.rounding(v[ok])
    tx = np.where(ok, round_away(np.where(ok, u, 0.0)), 0).astype(np.int64) - c0x + W
    ty = np.where(ok, round_away(np.where(ok, v, 0.0)), 0).astype(np.int64) - c0y + W
    ok &= (tx >= 0) & (tx < S) & (ty >= 0) & (ty < S)
    return np.where(ok, ty * S + tx, -1)


def parallel_pass(i, depths, colors, cams, overlap, processed, fused, *, max_depth_error, max_reproj_error, min_num_pixels,
                  max_traversal_depth=100):
    """Pass of view i of the committed parallel rule.  depths N x float32 [h,w], colors N x uint8 [h,w,3], cams [N,30], overlap
    N lists, processed N bools, fused N x uint8 [h,w] (NOT modified) -> dict: ``fused`` the masks after the pass, ``xyz``,
    ``normal`` float32 [M,3], ``rgb`` uint8 [M,3], ``pixel`` int [M] (seed order), ``margin``."""
    C = cam_rows(cams)
    n = len(depths)
    W = int(np.ceil(np.float32(max_reproj_error)))
    S, NB = 2 * W + 1, (2 * W + 1) ** 2
    e = float(np.float32(max_depth_error))
    r2 = float(np.float32(max_reproj_error)) ** 2
    adj = adjacency(overlap, n)
    margin = _Margin()
    dep = [np.asarray(d, dtype=np.float32) for d in depths]
    fz = [np.asarray(f, dtype=np.uint8) for f in fused]
    hi, wi = dep[i].shape
    di = dep[i].reshape(-1)
    seeds = np.nonzero(depth_ok(di) & (fz[i].reshape(-1) == 0))[0]
    ns = len(seeds)
    srow, scol = np.divmod(seeds, wi)
    Xs = unproject(C[i], scol.astype(np.float64), srow.astype(np.float64), di[seeds].astype(np.float64))
    act = [m != i and not processed[m] for m in range(n)]
    cand = np.zeros((ns, n, NB), dtype=bool)
    qidx = np.full((ns, n, NB), -1, dtype=np.int64)
    c0 = np.zeros((ns, n, 2), dtype=np.int64)
    Xn = np.zeros((ns, n, NB, 3), dtype=np.float64)
    for m in range(n):
        if not act[m]:
            continue
        hm, wm = dep[m].shape
        x, y, z = project(C[m], *Xs)
        with np.errstate(divide="ignore", invalid="ignore"):
            u, v = x / z, y / z
        okw = (z > 0) & (np.abs(u) < PIX_LIMIT) & (np.abs(v) < PIX_LIMIT)
        margin.rounding(u[okw])
        margin.rounding(v[okw])
        cx = np.where(okw, round_away(np.where(okw, u, 0.0)), 0).astype(np.int64)
        cy = np.where(okw, round_away(np.where(okw, v, 0.0)), 0).astype(np.int64)
        c0[:, m, 0], c0[:, m, 1] = cx, cy
        for b in range(NB):
            col, row = cx - W + b % S, cy - W + b // S
            inb = okw & (col >= 0) & (col < wm) & (row >= 0) & (row < hm)
            q = np.where(inb, row * wm + col, 0)
            dq = dep[m].reshape(-1)[q].astype(np.float64)
            live = inb & (fz[m].reshape(-1)[q] == 0) & depth_ok(dep[m].reshape(-1)[q])
            with np.errstate(divide="ignore", invalid="ignore"):
                derr = np.abs((z - dq) / dq)
                du, dv = u - col, v - row
                rerr = du * du + dv * dv
            margin.rel(derr[live], e)
            margin.rel(rerr[live], r2)
            ok = live & (derr <= e) & (rerr <= r2)
            cand[:, m, b] = ok
            qidx[:, m, b] = np.where(inb, q, -1)
            X = unproject(C[m], col.astype(np.float64), row.astype(np.float64), dq)
            Xn[:, m, b] = np.stack(X, axis=-1)

    def closure(cd):
        reach = np.zeros_like(cd)
        if max_traversal_depth < 2:
            return reach
        for m in np.nonzero(adj[i])[0]:
            if not act[m]:
                continue
            t = _target(C[m], *Xs, c0[:, m, 0], c0[:, m, 1], W, margin)
            hit = (t >= 0) & cd[np.arange(ns), m, np.maximum(t, 0)]
            reach[np.nonzero(hit)[0], m, t[hit]] = True
        front = reach.copy()
        lvl = 1
        while lvl + 1 <= max_traversal_depth - 1 and front.any():
            fs, fk, fb = np.nonzero(front)
            X = Xn[fs, fk, fb]
            nxt = np.zeros_like(cd)
            for m in range(n):
                if not act[m]:
                    continue
                sel = adj[fk, m]
                if not sel.any():
                    continue
                ss = fs[sel]
                t = _target(C[m], X[sel, 0], X[sel, 1], X[sel, 2], c0[ss, m, 0], c0[ss, m, 1], W, margin)
                hit = (t >= 0) & cd[ss, m, np.maximum(t, 0)] & ~reach[ss, m, np.maximum(t, 0)]
                nxt[ss[hit], m, t[hit]] = True
            reach |= nxt
            front = nxt
            lvl += 1
        return reach

    reach_a = closure(cand)
    claim = [np.full(d.size, np.iinfo(np.int64).max, dtype=np.int64) for d in dep]
    ss, mm, bb = np.nonzero(reach_a)
    for m in range(n):
        sel = mm == m
        np.minimum.at(claim[m], qidx[ss[sel], m, bb[sel]], seeds[ss[sel]])
    own = np.zeros_like(cand)
    for m in range(n):
        if act[m]:
            q = qidx[:, m, :]
            own[:, m, :] = reach_a[:, m, :] & (claim[m][np.maximum(q, 0)] == seeds[:, None])
    reach_b = closure(own)

    new_fused = [f.copy().reshape(-1) for f in fz]
    new_fused[i][seeds] = 1
    ss, mm, bb = np.nonzero(reach_b)
    for m in range(n):
        sel = mm == m
        new_fused[m][qidx[ss[sel], m, bb[sel]]] = 1
    nrm = [view_normal(C[v]) for v in range(n)]
    pts, nors, rgbs, pix = [], [], [], []
    cols = [np.asarray(c, dtype=np.uint8).reshape(-1, 3) for c in colors]
    counts = 1 + reach_b.sum(axis=(1, 2))
    for k in np.nonzero(counts >= min_num_pixels)[0]:
        _, m_, b_ = np.nonzero(reach_b[k:k + 1])
        xyz = np.concatenate([np.array(Xs)[:, k][None], Xn[k, m_, b_]], axis=0).astype(np.float32)
        nor = np.stack([nrm[i]] + [nrm[m] for m in m_])
        col = np.concatenate([cols[i][seeds[k]][None], np.stack([cols[m][qidx[k, m, b]] for m, b in zip(m_, b_)])
                              if len(m_) else np.zeros((0, 3), np.uint8)], axis=0)
        p = emit_point(xyz, nor, col)
        if p is None:
            continue
        pts.append(p[0]); nors.append(p[1]); rgbs.append(p[2]); pix.append(int(seeds[k]))
    cat = lambda a, dt: np.stack(a).astype(dt) if a else np.zeros((0, 3), dt)
    return {"fused": [f.reshape(d.shape) for f, d in zip(new_fused, dep)], "xyz": cat(pts, np.float32),
            "normal": cat(nors, np.float32), "rgb": cat(rgbs, np.uint8), "pixel": np.array(pix, dtype=np.int64),
            "margin": margin.v}


def parallel_fuse(depths, colors, cams, overlap, **kw):
    """All passes in FindNextImage order -> (xyz, normal, rgb, view, margin, per-pass results)."""
    n = len(depths)
    fused = [np.zeros(np.shape(d), np.uint8) for d in depths]
    processed = [False] * n
    out, passes, margin = [], [], np.inf
    for v in find_next_image_order(overlap):
        r = parallel_pass(v, depths, colors, cams, overlap, processed, fused, **kw)
        fused = r["fused"]
        processed[v] = True
        margin = min(margin, r["margin"])
        out.append((r["xyz"], r["normal"], r["rgb"], np.full(len(r["pixel"]), v, np.int32)))
        passes.append((v, r))
    xyz, nor, rgb, view = (np.concatenate([o[k] for o in out]) for k in range(4))
    return xyz, nor, rgb, view, margin, passes


def sequential_fuse(depths, colors, cams, overlap, *, max_depth_error, max_reproj_error, min_num_pixels, max_traversal_depth=100,
                    max_num_pixels=10000):
    """COLMAP's StereoFusion as recalled in INTEGRATION.md section 2g, literally: one seed at a time, a FIFO traversal that marks
    accepted pixels at once, may enter the seed's own view, and follows overlap[k] in list order.  Pure Python: small scenes only."""
    C = cam_rows(cams)
    n = len(depths)
    dep = [np.asarray(d, dtype=np.float32) for d in depths]
    cols = [np.asarray(c, dtype=np.uint8) for c in colors]
    fused = [np.zeros(d.shape, bool) for d in dep]
    processed = [False] * n
    e = float(np.float32(max_depth_error))
    r2 = float(np.float32(max_reproj_error)) ** 2
    nrm = [view_normal(C[v]) for v in range(n)]
    pts, nors, rgbs, views = [], [], [], []
    for i in find_next_image_order(overlap):
        h, w = dep[i].shape
        for row in range(h):
            for col in range(w):
                if fused[i][row, col] or not depth_ok(dep[i][row, col]):
                    continue
                queue = deque([(i, row, col, 0)])
                ref = None
                xyz, nor, rgb = [], [], []
                while queue:
                    k, r_, c_, td = queue.popleft()
                    if fused[k][r_, c_]:
                        continue
                    d = dep[k][r_, c_]
                    if not depth_ok(d):
                        continue
                    if td > 0:
                        x, y, z = project(C[k], *ref)
                        if not abs((z - float(d)) / float(d)) <= e:
                            continue
                        du, dv = x / z - c_, y / z - r_
                        if not du * du + dv * dv <= r2:
                            continue
                    X = unproject(C[k], float(c_), float(r_), float(d))
                    fused[k][r_, c_] = True
                    xyz.append(X); nor.append(nrm[k]); rgb.append(cols[k][r_, c_])
                    if td == 0:
                        ref = X
                    if len(xyz) >= max_num_pixels:
                        break
                    if td + 1 >= max_traversal_depth:
                        continue
                    for m in overlap[k]:
                        if processed[m] or m == k:
                            continue
                        hm, wm = dep[m].shape
                        x, y, z = project(C[m], *X)
                        if z == 0:
                            continue
                        nc, nr = round_away(x / z), round_away(y / z)
                        if 0 <= nc < wm and 0 <= nr < hm:
                            queue.append((m, int(nr), int(nc), td + 1))
                if len(xyz) >= min_num_pixels:
                    p = emit_point(np.array(xyz, dtype=np.float64).astype(np.float32), np.stack(nor), np.stack(rgb))
                    if p is not None:
                        pts.append(p[0]); nors.append(p[1]); rgbs.append(p[2]); views.append(i)
        processed[i] = True
    cat = lambda a, dt: np.stack(a).astype(dt) if a else np.zeros((0, 3), dt)
    return cat(pts, np.float32), cat(nors, np.float32), cat(rgbs, np.uint8), np.array(views, np.int32)


def chamfer(a, b):
    """Mean of the two directed mean nearest-neighbour distances (brute force, float64)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)

    def directed(p, q):
        out = np.empty(len(p))
        for s in range(0, len(p), 512):
            d = ((p[s:s + 512, None, :] - q[None, :, :]) ** 2).sum(-1)
            out[s:s + 512] = np.sqrt(d.min(axis=1))
        return out.mean()

    return 0.5 * (directed(a, b) + directed(b, a))
