"""numpy restatement of the scene set-up from a COLMAP sparse model, the yardstick of
csrc/scene_setup.hip, and the synthetic scenes its tests and its benchmark share.

``pair_counts`` loops over the points and works only on the pairs of each track (the reference builds dense N x N arrays per
point); geometry is float64 from the float32 R and t, in the kernel's form c[i,j] = R_i (R_j^T t_j) - t_i of the reference's
``rel_opt_center``.  Next to the matrices it returns the smallest distance of any off-diagonal pair's angle to the threshold: a
pair that close could be decided the other way by a last-bit difference (tests/golden/gen_golden_scene.py asserts 1e-3 degrees
for the fixture, where the reference itself, with its float32 products, is the yardstick).
``depth_ranges`` is the reference's float64 rule (no float32 rounding of the depths): ``np.percentile`` per image."""
from __future__ import annotations

import numpy as np


def flatten_model(images, points3d):
    """(xyz [P,3], track_off [P+1], track_img [nnz], obs_img [M], obs_pt [M]) of a sparse model given as dicts of namedtuples:
    image indices are positions in ``images``, tracks sorted and de-duplicated per point, observations image by image."""
    index = {im_id: k for k, im_id in enumerate(images)}
    row = {pid: k for k, pid in enumerate(points3d)}
    xyz = np.array([p.xyz for p in points3d.values()], dtype=np.float64).reshape(-1, 3)
    tracks = [sorted({index[i] for i in np.asarray(p.image_ids).tolist()}) for p in points3d.values()]
    off = np.zeros(len(tracks) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(tr) for tr in tracks])
    img = np.array([i for tr in tracks for i in tr], dtype=np.int32)
    obs_img, obs_pt = [], []
    for k, im in enumerate(images.values()):
        for p in np.asarray(im.point3D_ids).tolist():
            if p != -1:
                obs_img.append(k)
                obs_pt.append(row[p])
    return xyz, off, img, np.array(obs_img, dtype=np.int32), np.array(obs_pt, dtype=np.int32)


def pair_counts(xyz, track_off, track_img, R, t, min_triangulation_angle):
    """-> (adj int64 [N,N], adj_tri int64 [N,N], margin): ``adj[i,j]`` the points whose track holds i and j (diagonal included),
    ``adj_tri[i,j]`` those with angle(x, x + c[i,j]) > min_triangulation_angle degrees (never on the diagonal); ``margin`` the
    smallest |angle - threshold| over all off-diagonal pairs (inf without any)."""
    R = np.asarray(R, dtype=np.float32).reshape(-1, 3, 3).astype(np.float64)
    t = np.asarray(t, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    n = len(R)
    w = np.einsum("nji,nj->ni", R, t)                                   # R_j^T t_j
    adj = np.zeros((n, n), dtype=np.int64)
    adj_tri = np.zeros((n, n), dtype=np.int64)
    margin = np.inf
    for p in range(len(track_off) - 1):
        idx = np.asarray(track_img[track_off[p]:track_off[p + 1]], dtype=np.int64)
        if len(idx) == 0:
            continue
        x = np.asarray(xyz[p], dtype=np.float64)
        c = np.einsum("aij,bj->abi", R[idx], w[idx]) - t[idx][:, None, :]       # [a, b]: from a = row to b = column
        ray2 = x + c
        with np.errstate(all="ignore"):
            cos = np.clip((x * ray2).sum(-1) / np.linalg.norm(x) / np.linalg.norm(ray2, axis=-1), -1, 1)
            angle = np.arccos(cos) / np.pi * 180
        off_diag = ~np.eye(len(idx), dtype=bool)
        tri = (angle > min_triangulation_angle) & off_diag
        adj[np.ix_(idx, idx)] += 1
        adj_tri[np.ix_(idx, idx)] += tri
        if off_diag.any():
            with np.errstate(all="ignore"):
                margin = min(margin, float(np.nanmin(np.abs(angle - min_triangulation_angle)[off_diag])))
    return adj, adj_tri, margin


def select(adj, adj_tri, nsrc):
    """The reference's choice, row by row: zero where adj_tri < 0.75 adj, stable ascending argsort, the last ``nsrc`` indices."""
    out = []
    for i in range(adj.shape[0]):
        common = adj[i].copy()
        common[4 * adj_tri[i] < 3 * adj[i]] = 0
        out.append(np.argsort(common, kind="stable")[-nsrc:].tolist())
    return out


def depth_ranges(xyz, obs_img, obs_pt, R, t, perc=(1, 99)):
    """-> (depth_min, depth_max) float64 [N]: percentiles of (R_i x + t_i).z + 1e-6 over image i's observations, 0 and 0 without."""
    R = np.asarray(R, dtype=np.float32).reshape(-1, 3, 3).astype(np.float64)
    t = np.asarray(t, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    lo, hi = np.zeros(len(R)), np.zeros(len(R))
    for i in range(len(R)):
        pts = np.asarray(xyz, dtype=np.float64)[np.asarray(obs_pt)[np.asarray(obs_img) == i]]
        if len(pts):
            lo[i], hi[i] = np.percentile((pts @ R[i].T + t[i])[:, 2] + 1e-6, perc)
    return lo, hi


def scene_setup(images, points3d, R, t, *, min_triangulation_angle, nsrc, perc=(1, 99)):
    """Everything at once from a model: dict(adj, adj_tri, margin, sel_idx, depth_min, depth_max)."""
    xyz, off, img, obs_img, obs_pt = flatten_model(images, points3d)
    adj, adj_tri, margin = pair_counts(xyz, off, img, R, t, min_triangulation_angle)
    lo, hi = depth_ranges(xyz, obs_img, obs_pt, R, t, perc)
    return dict(adj=adj, adj_tri=adj_tri, margin=margin, sel_idx=select(adj, adj_tri, nsrc), depth_min=lo, depth_max=hi)


# ---- synthetic scenes (arrays only) --------------------------------------------------------------------------------------------
def rig(n_images, rng, spacing):
    """Cameras on a jittered grid in the plane z = 0, looking along +z with a small random rotation: (R fp32 [N,3,3], t fp32 [N,3])."""
    side = int(np.ceil(np.sqrt(n_images)))
    centre = np.stack([(np.arange(n_images) % side - (side - 1) / 2) * spacing, (np.arange(n_images) // side - (side - 1) / 2) * spacing,
                       np.zeros(n_images)], axis=1) + rng.normal(0, 0.1 * spacing, (n_images, 3))
    q = np.concatenate([np.ones((n_images, 1)), rng.normal(0, 0.03, (n_images, 3))], axis=1)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, v = q[:, 0], q[:, 1:]                                            # R = (w^2 - v.v) I + 2 v v^T + 2 w [v]_x
    cross = np.zeros((n_images, 3, 3))
    cross[:, 0, 1], cross[:, 0, 2], cross[:, 1, 2] = -v[:, 2], v[:, 1], -v[:, 0]
    cross -= cross.transpose(0, 2, 1)
    R = ((w * w - (v * v).sum(1))[:, None, None] * np.eye(3) + 2 * v[:, :, None] * v[:, None, :] + 2 * w[:, None, None] * cross)
    t = -np.einsum("nij,nj->ni", R, centre)
    return R.astype(np.float32), t.astype(np.float32)


def synthetic_scene(n_images, n_points, lengths, seed, spacing=0.3):
    """A scene as arrays: points in a box 3..7 in front of the rig, point p seen by ``lengths[p]`` distinct images (a window of
    neighbouring image indices around a random one, so that tracks overlap), every image's observations = its tracks.
    -> dict(xyz, track_off, track_img, obs_img, obs_pt, R, t)."""
    rng = np.random.default_rng(seed)
    R, t = rig(n_images, rng, spacing)
    lengths = np.minimum(np.asarray(lengths, dtype=np.int64), n_images)
    xyz = np.stack([rng.uniform(-2, 2, n_points), rng.uniform(-2, 2, n_points), rng.uniform(3, 7, n_points)], axis=1)
    off = np.zeros(n_points + 1, dtype=np.int64)
    off[1:] = np.cumsum(lengths)
    img = np.empty(off[-1], dtype=np.int32)
    start = rng.integers(0, n_images, n_points)
    for p in range(n_points):
        pool = (start[p] + np.arange(min(n_images, 2 * lengths[p]))) % n_images
        img[off[p]:off[p + 1]] = np.sort(rng.choice(pool, lengths[p], replace=False))
    obs_pt = np.repeat(np.arange(n_points, dtype=np.int32), lengths)
    return dict(xyz=xyz, track_off=off, track_img=img, obs_img=img.copy(), obs_pt=obs_pt, R=R, t=t)


def heavy_tailed_lengths(n_points, mean, longest, seed):
    """Track lengths >= 2 from a Pareto tail (shape 1.5) scaled to the given mean, capped at ``longest``."""
    rng = np.random.default_rng(seed)
    raw = 2 + rng.pareto(1.5, n_points) * (mean - 2) * 0.5
    return np.clip(np.round(raw), 2, longest).astype(np.int64)


def bench_scene(n_images=2000, n_points=300000, mean=8.0, seed=0):
    """The scene of scripts/bench_scene_setup.py and scripts/time_reference_cpu.py --scene-setup."""
    return synthetic_scene(n_images, n_points, heavy_tailed_lengths(n_points, mean, n_images, seed), seed)


def scene_70():
    """The second GPU case: 70 images, 2 000 points, tracks of 2..70 images (some longer than one wave of 64 lanes, two of them
    of all 70 images), N not a multiple of anything the kernel tiles by."""
    rng = np.random.default_rng(7)
    lengths = np.concatenate([[70, 70, 69, 66, 65, 64, 63], rng.integers(2, 40, 2000 - 7)])
    return synthetic_scene(70, 2000, lengths, seed=70)
