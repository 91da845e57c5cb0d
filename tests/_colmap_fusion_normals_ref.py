"""numpy restatement of the COLMAP-style stereo fusion WITH NORMAL MAPS ("with normal maps"), the
yardstick of the NORMALS = true kernels of csrc/colmap_fusion.hip, and COLMAP's sequential loop with the normal test at its place
(after the depth and reprojection tests, before the pixel is marked).

The geometry helpers are those of tests/_colmap_fusion_ref.py.  A pixel's world normal is R^T n, float64 sums of three products
in the kernel's order, rounded to float32; the test ``w_seed . w_pixel >= min_cos`` is a float64 sum in x, y, z order.
``parallel_pass`` reports ``margin`` as the normal-free rule does, also over ``|dot - min_cos| / max(|min_cos|, 1e-3)`` of every
pair that reached the normal test, and ``tested`` / ``rejected``: the (seed, pixel) pairs that passed depth and reprojection, and
those of them the normal test refused."""
from __future__ import annotations

from collections import deque

import numpy as np

from tests._colmap_fusion_ref import (PIX_LIMIT, _Margin, _target, adjacency, depth_ok, emit_point, find_next_image_order, project,
                                      round_away, unproject)
from tests._fusion_ref import cam_rows


def min_cos_of(max_normal_error):
    """cos(max_normal_error_fp32 * pi / 180) in float64, as the C entry point computes it."""
    return float(np.cos(np.float64(np.float32(max_normal_error)) * 3.14159265358979323846 / 180.0))


def world_normals(c, normal):
    """fp32 [..., 3] camera-frame normals of the view with float64 camera row c -> R^T n, float32 [..., 3]."""
    n = np.asarray(normal, dtype=np.float32).astype(np.float64)
    nx, ny, nz = n[..., 0], n[..., 1], n[..., 2]
    return np.stack([c[18] * nx + c[21] * ny + c[24] * nz, c[19] * nx + c[22] * ny + c[25] * nz,
                     c[20] * nx + c[23] * ny + c[26] * nz], axis=-1).astype(np.float32)


def _dot(a, b):
    """float64 a.x b.x + a.y b.y + a.z b.z of float32 [..., 3] arrays, summed in that order."""
    a, b = a.astype(np.float64), b.astype(np.float64)
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def parallel_pass(i, depths, colors, normals, cams, overlap, processed, fused, *, max_depth_error, max_reproj_error, min_num_pixels,
                  max_normal_error, max_traversal_depth=100):
    """Pass of view i of the parallel rule with normal maps.  As ``_colmap_fusion_ref.parallel_pass``, plus normals N x float32
    [h,w,3] (camera frame) and max_normal_error (degrees) -> the same dict, plus ``tested`` and ``rejected``."""
    C = cam_rows(cams)
    n = len(depths)
    W = int(np.ceil(np.float32(max_reproj_error)))
    S, NB = 2 * W + 1, (2 * W + 1) ** 2
    e = float(np.float32(max_depth_error))
    r2 = float(np.float32(max_reproj_error)) ** 2
    min_cos = min_cos_of(max_normal_error)
    adj = adjacency(overlap, n)
    margin = _Margin()
    dep = [np.asarray(d, dtype=np.float32) for d in depths]
    fz = [np.asarray(f, dtype=np.uint8) for f in fused]
    wn = [world_normals(C[v], np.asarray(normals[v], dtype=np.float32).reshape(-1, 3)) for v in range(n)]
    hi, wi = dep[i].shape
    di = dep[i].reshape(-1)
    seeds = np.nonzero(depth_ok(di) & (fz[i].reshape(-1) == 0))[0]
    ns = len(seeds)
    srow, scol = np.divmod(seeds, wi)
    Xs = unproject(C[i], scol.astype(np.float64), srow.astype(np.float64), di[seeds].astype(np.float64))
    ws = wn[i][seeds]
    act = [m != i and not processed[m] for m in range(n)]
    cand = np.zeros((ns, n, NB), dtype=bool)
    qidx = np.full((ns, n, NB), -1, dtype=np.int64)
    c0 = np.zeros((ns, n, 2), dtype=np.int64)
    Xn = np.zeros((ns, n, NB, 3), dtype=np.float64)
    tested = rejected = 0
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
                dot = _dot(ws, wn[m][q])
            margin.rel(derr[live], e)
            margin.rel(rerr[live], r2)
            geo = live & (derr <= e) & (rerr <= r2)
            sel = geo & np.isfinite(dot)
            if sel.any():
                margin.v = min(margin.v, float(np.min(np.abs(dot[sel] - min_cos))) / max(abs(min_cos), 1e-3))
            ok = geo & (dot >= min_cos)                                     # (NaN fails)
            tested += int(geo.sum())
            rejected += int((geo & ~ok).sum())
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
    pts, nors, rgbs, pix = [], [], [], []
    cols = [np.asarray(c, dtype=np.uint8).reshape(-1, 3) for c in colors]
    counts = 1 + reach_b.sum(axis=(1, 2))
    for k in np.nonzero(counts >= min_num_pixels)[0]:
        _, m_, b_ = np.nonzero(reach_b[k:k + 1])
        xyz = np.concatenate([np.array(Xs)[:, k][None], Xn[k, m_, b_]], axis=0).astype(np.float32)
        nor = np.stack([ws[k]] + [wn[m][qidx[k, m, b]] for m, b in zip(m_, b_)])
        col = np.concatenate([cols[i][seeds[k]][None], np.stack([cols[m][qidx[k, m, b]] for m, b in zip(m_, b_)])
                              if len(m_) else np.zeros((0, 3), np.uint8)], axis=0)
        p = emit_point(xyz, nor, col)
        if p is None:
            continue
        pts.append(p[0]); nors.append(p[1]); rgbs.append(p[2]); pix.append(int(seeds[k]))
    cat = lambda a, dt: np.stack(a).astype(dt) if a else np.zeros((0, 3), dt)
    return {"fused": [f.reshape(d.shape) for f, d in zip(new_fused, dep)], "xyz": cat(pts, np.float32),
            "normal": cat(nors, np.float32), "rgb": cat(rgbs, np.uint8), "pixel": np.array(pix, dtype=np.int64),
            "margin": margin.v, "tested": tested, "rejected": rejected}


def parallel_fuse(depths, colors, normals, cams, overlap, **kw):
    """All passes in FindNextImage order -> (xyz, normal, rgb, view, margin, per-pass results)."""
    n = len(depths)
    fused = [np.zeros(np.shape(d), np.uint8) for d in depths]
    processed = [False] * n
    out, passes, margin = [], [], np.inf
    for v in find_next_image_order(overlap):
        r = parallel_pass(v, depths, colors, normals, cams, overlap, processed, fused, **kw)
        fused = r["fused"]
        processed[v] = True
        margin = min(margin, r["margin"])
        out.append((r["xyz"], r["normal"], r["rgb"], np.full(len(r["pixel"]), v, np.int32)))
        passes.append((v, r))
    xyz, nor, rgb, view = (np.concatenate([o[k] for o in out]) for k in range(4))
    return xyz, nor, rgb, view, margin, passes


def sequential_fuse(depths, colors, normals, cams, overlap, *, max_depth_error, max_reproj_error, min_num_pixels, max_normal_error,
                    max_traversal_depth=100, max_num_pixels=10000):
    """COLMAP's StereoFusion loop as ``_colmap_fusion_ref.sequential_fuse`` restates it, with the normal test where COLMAP has it:
    after the depth and reprojection tests of a node at traversal depth > 0, against the seed's normal (fused_ref_normal), and
    before the pixel is marked.  Pure Python: small scenes only."""
    C = cam_rows(cams)
    n = len(depths)
    dep = [np.asarray(d, dtype=np.float32) for d in depths]
    cols = [np.asarray(c, dtype=np.uint8) for c in colors]
    wn = [world_normals(C[v], np.asarray(normals[v], dtype=np.float32)) for v in range(n)]
    fused = [np.zeros(d.shape, bool) for d in dep]
    processed = [False] * n
    e = float(np.float32(max_depth_error))
    r2 = float(np.float32(max_reproj_error)) ** 2
    min_cos = min_cos_of(max_normal_error)
    pts, nors, rgbs, views = [], [], [], []
    for i in find_next_image_order(overlap):
        h, w = dep[i].shape
        for row in range(h):
            for col in range(w):
                if fused[i][row, col] or not depth_ok(dep[i][row, col]):
                    continue
                queue = deque([(i, row, col, 0)])
                ref = ref_normal = None
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
                    normal = wn[k][r_, c_]
                    if td > 0 and not float(_dot(ref_normal, normal)) >= min_cos:
                        continue
                    X = unproject(C[k], float(c_), float(r_), float(d))
                    fused[k][r_, c_] = True
                    xyz.append(X); nor.append(normal); rgb.append(cols[k][r_, c_])
                    if td == 0:
                        ref, ref_normal = X, normal
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
