"""numpy restatement of the depth-map fusion rule, the yardstick of csrc/depth_fusion.hip, and of the
reference's ``utils/utils_ply.py:read_ply`` for the binary files the fusion step writes.

Geometry is evaluated in float64 from the float32 inputs the kernel reads (depth maps, camera blocks [N,30] = K, K^-1, R, t, and the
three thresholds as fp32 numbers), so the kernel's fp32 rounding is the only difference.  This is the plain statement of the rule;
the kernel is held to tests/_fusion_bounds.py, which restates it with a derived rounding bound per step and evaluates every decision
over its interval."""
from __future__ import annotations

import numpy as np

PLY_DTYPES = {b"float32": "f4", b"float": "f4", b"uint8": "u1", b"uchar": "u1", b"int32": "i4", b"float64": "f8"}


def read_ply(path):
    """Structured array of a binary PLY file (what the reference's read_ply returns)."""
    with open(path, "rb") as fh:
        if b"ply" not in fh.readline():
            raise ValueError("not a ply file")
        fmt = fh.readline().split()[1].decode()
        ext = {"binary_little_endian": "<", "binary_big_endian": ">"}[fmt]
        props, n, line = [], None, b""
        while b"end_header" not in line:
            line = fh.readline()
            if line == b"":
                raise ValueError("truncated header")
            if b"element" in line:
                n = int(line.split()[2])
            elif b"property" in line:
                tok = line.split()
                props.append((tok[2].decode(), ext + PLY_DTYPES[tok[1]]))
        return np.fromfile(fh, dtype=props, count=n)


def cam_rows(cams):
    """Camera blocks [N,30] (K, K^-1, R, t) as float64 rows of their fp32 values."""
    return np.asarray(cams, dtype=np.float32).astype(np.float64)


def cam_parts(cams):
    c = cam_rows(cams)
    K, Ki, R, t = c[:, 0:9].reshape(-1, 3, 3), c[:, 9:18].reshape(-1, 3, 3), c[:, 18:27].reshape(-1, 3, 3), c[:, 27:30]
    return K, Ki, R, t


def valid(d, lo, hi):
    """finite and float32(lo) < d < float32(hi): the kernel holds its thresholds as fp32 numbers, so a depth equal to float32(1e-3),
    which exceeds the double 1e-3, is not valid"""
    return np.isfinite(d) & (d > float(np.float32(lo))) & (d < float(np.float32(hi)))


def unproject(Ki, R, t, x, y, d):
    """R^T (d K^-1 (x, y, 1) - t) for arrays of pixels -> [..., 3]."""
    p = np.stack((x * d, y * d, d), axis=-1) @ Ki.T
    return (p - t) @ R


def fuse_pass(i, depths, colors, cams, used, *, disp_thresh, num_consistent, depth_min=1e-3, depth_max=1e5):
    """Pass i of the rule.  depths N x float32 [h,w], colors N x uint8 [h,w,3], cams [N,30], used N x uint8 [h,w] (NOT modified)
    -> dict: ``emit`` bool [h_i,w_i], ``xyz`` [h_i,w_i,3], ``rgb`` int [h_i,w_i,3] (valid where emit), ``n`` consistent views,
    ``used`` the N masks after the pass, ``hits`` (j, consistent [h_i,w_i], qx, qy) per other view."""
    K, Ki, R, t = cam_parts(cams)
    N = len(depths)
    d = np.asarray(depths[i], dtype=np.float32).astype(np.float64)
    h, w = d.shape
    ys, xs = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    active = valid(d, depth_min, depth_max) & (np.asarray(used[i]) == 0)
    X = unproject(Ki[i], R[i], t[i], xs, ys, np.where(active, d, 0.0))
    centre = -np.einsum("nji,nj->ni", R, t)
    f_i = K[i, 0, 0]
    S = np.zeros((h, w, 3))
    csum = np.asarray(colors[i]).astype(np.int64).copy()
    n = np.zeros((h, w), dtype=np.int64)
    hits = []
    for j in range(N):
        if j == i:
            continue
        hj, wj = depths[j].shape
        P = (X @ R[j].T + t[j]) @ K[j].T
        z = P[..., 2]
        front = active & (z > 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            u, v = P[..., 0] / z, P[..., 1] / z
        fx, fy = np.floor(u + 0.5), np.floor(v + 0.5)
        inb = front & (fx >= 0) & (fx < wj) & (fy >= 0) & (fy < hj)
        qx, qy = np.where(inb, fx, 0).astype(np.int64), np.where(inb, fy, 0).astype(np.int64)
        dj = np.asarray(depths[j], dtype=np.float32).astype(np.float64)[qy, qx]
        ok = inb & valid(dj, depth_min, depth_max)
        fb = f_i * np.linalg.norm(centre[i] - centre[j])
        with np.errstate(divide="ignore", invalid="ignore"):
            disp = np.abs(fb / z - fb / dj)
        cons = ok & (disp < float(np.float32(disp_thresh)))           # (the threshold as the kernel holds it: an fp32 number)
        Xj = unproject(Ki[j], R[j], t[j], qx.astype(np.float64), qy.astype(np.float64), dj)
        S += np.where(cons[..., None], Xj, 0.0)
        csum += np.where(cons[..., None], np.asarray(colors[j])[qy, qx].astype(np.int64), 0)
        n += cons
        hits.append((j, cons, qx, qy))
    emit = active & (n >= num_consistent)
    xyz = (X + S) / (n + 1)[..., None]
    rgb = np.floor(csum / (n + 1)[..., None] + 0.5).astype(np.int64)
    after = [np.asarray(u_).copy() for u_ in used]
    for j, cons, qx, qy in hits:
        m = emit & cons
        after[j][qy[m], qx[m]] = 1
    return {"emit": emit, "xyz": xyz, "rgb": rgb, "n": n, "used": after, "hits": hits}


def fuse_all(depths, colors, cams, **kw):
    """Every pass in order -> (xyz [M,3], rgb [M,3], view [M], pixel [M]) in the kernel's output order, plus the per-pass results."""
    used = [np.zeros(np.asarray(d).shape, dtype=np.uint8) for d in depths]
    pts, cols, views, pix, passes = [], [], [], [], []
    for i in range(len(depths)):
        r = fuse_pass(i, depths, colors, cams, used, **kw)
        used = r["used"]
        idx = np.flatnonzero(r["emit"].reshape(-1))
        pts.append(r["xyz"].reshape(-1, 3)[idx])
        cols.append(r["rgb"].reshape(-1, 3)[idx])
        views.append(np.full(idx.shape, i, dtype=np.int64))
        pix.append(idx)
        passes.append(r)
    return np.concatenate(pts), np.concatenate(cols), np.concatenate(views), np.concatenate(pix), passes
