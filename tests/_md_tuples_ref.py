"""numpy restatement of the MegaDepth tuple mining: the visible depth range of an image tuple, the
yardstick of pscv_tuple_visible_depths (csrc/scene_setup.hip), and the control flow of the miner
(wild_deep_mvs_amd/preprocess.py), plus the synthetic scenes its tests and its benchmark share.

``visible_depths`` works on the flattened model (tests/_scene_setup_ref.py:flatten_model): a point takes part in a tuple when
at least 3 of the tuple's images are in its track; it is projected into every view in float64 from the float32 K, R, t
(y = R x + t, u = K y, depth = u_z + 1e-6, proj = u_xy / depth) and is valid where 0 <= proj < (w, h) and depth > 0.  Per view the
smallest and largest valid depth and the first (lowest) row that attains each; NaN and -1 for a view without a valid point.  It
also returns, per view, the magnitude M = sum_k |K_3. R_.k x_k| + |K_3. t| + 1e-6 of the two attaining points: two float64
evaluations of a depth differ by summation order only, a few ulp of M.
``mine`` is the miner's loop over reference images, candidates and tuples, from the two count matrices."""
from __future__ import annotations

import numpy as np


def resized_size(size, min_size):
    """(width, height) after scaling the shorter side to ``min_size`` and cutting both down to multiples of 32."""
    w, h = size
    ratio = min(w / min_size, h / min_size)
    return int(w / ratio / 32) * 32, int(h / ratio / 32) * 32


def visible_depths(xyz, track_off, track_img, tup, K, R, t, sizes):
    """One tuple: ``tup`` [V] image indices, K [V,3,3], R [N,3,3], t [N,3] of ALL images, sizes [V,2] = (w, h) ->
    dict(min_d [V], max_d [V], min_row [V], max_row [V], n_pts, M_min [V], M_max [V])."""
    tup = np.asarray(tup, dtype=np.int64)
    V = len(tup)
    K = np.asarray(K, dtype=np.float32).reshape(V, 3, 3).astype(np.float64)
    R = np.asarray(R, dtype=np.float32).reshape(-1, 3, 3).astype(np.float64)[tup]
    t = np.asarray(t, dtype=np.float32).reshape(-1, 3).astype(np.float64)[tup]
    sizes = np.asarray(sizes, dtype=np.float64).reshape(V, 2)
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    member = np.zeros(int(max(np.max(track_img, initial=0), tup.max())) + 1, dtype=np.int64)
    member[tup] = 1
    hits = np.zeros(len(xyz), dtype=np.int64)
    np.add.at(hits, np.repeat(np.arange(len(xyz)), np.diff(track_off)), member[np.asarray(track_img, dtype=np.int64)])
    rows = np.nonzero(hits >= 3)[0]
    out = dict(min_d=np.full(V, np.nan), max_d=np.full(V, np.nan), min_row=np.full(V, -1, dtype=np.int64),
               max_row=np.full(V, -1, dtype=np.int64), n_pts=len(rows), M_min=np.full(V, 1e-6), M_max=np.full(V, 1e-6))
    if len(rows) == 0:
        return out
    x = xyz[rows]                                                        # [n,3]
    # element by element, left to right (no matrix product: the same input gives the same bits wherever it stands in the array)
    dot = lambda A, b: A[:, None, :, 0] * b[..., 0, None] + A[:, None, :, 1] * b[..., 1, None] + A[:, None, :, 2] * b[..., 2, None]
    y = dot(R, x[None]) + t[:, None, :]                                  # [V,n,3]
    u = dot(K, y)
    depth = u[..., 2] + 1e-6
    with np.errstate(all="ignore"):
        proj = u[..., :2] / depth[..., None]
        valid = ((proj[..., 0] >= 0) & (proj[..., 1] >= 0) & (proj[..., 0] < sizes[:, 0, None]) & (proj[..., 1] < sizes[:, 1, None])
                 & (depth > 0))
    k3r = np.einsum("vj,vjk->vk", K[:, 2], R)                            # K's third row times R
    M = np.abs(k3r[:, None, :] * x[None]).sum(-1) + np.abs((K[:, 2] * t).sum(-1))[:, None] + 1e-6           # [V,n]
    for v in range(V):
        if valid[v].any():
            d = np.where(valid[v], depth[v], np.nan)
            lo, hi = int(np.nanargmin(d)), int(np.nanargmax(d))          # the first among equals
            out["min_d"][v], out["max_d"][v] = d[lo], d[hi]
            out["min_row"][v], out["max_row"][v] = rows[lo], rows[hi]
            out["M_min"][v], out["M_max"][v] = M[v, lo], M[v, hi]
    return out


def visible_depths_batch(xyz, track_off, track_img, tuples, K, R, t, sizes):
    """Many tuples: tuples [T,V], K [T,V,3,3], sizes [T,V,2] -> dict of stacked arrays (n_pts [T], the others [T,V])."""
    res = [visible_depths(xyz, track_off, track_img, tuples[k], K[k], R, t, sizes[k]) for k in range(len(tuples))]
    return {key: np.stack([np.asarray(r[key]) for r in res]) for key in res[0]}


def visible_range(xyz, track_off, track_img, tup, K, R, t, sizes):
    """What compute_min_max_depth_visible returns: (min_d, max_d, min_point, max_point), or four None when no point takes part or
    a view has no valid point."""
    r = visible_depths(xyz, track_off, track_img, tup, K, R, t, sizes)
    if r["n_pts"] == 0 or (r["min_row"] < 0).any():
        return None, None, None, None
    xyz = np.asarray(xyz, dtype=np.float64)
    return r["min_d"], r["max_d"], xyz[r["min_row"]], xyz[r["max_row"]]


def rescaled(K, image_sizes, idx_list, min_size=512):
    """The tuple's intrinsics and sizes after the resize to ``min_size``: float32 rows 0 and 1 of K times new / old width and height."""
    newK = np.asarray(K, dtype=np.float32)[idx_list].copy()
    new_sizes = []
    for k, i in enumerate(idx_list):
        w, h = int(image_sizes[i][0]), int(image_sizes[i][1])
        rw, rh = resized_size((w, h), min_size)
        new_sizes.append((rw, rh))
        newK[k][0:1] *= rw / w
        newK[k][1:2] *= rh / h
    return newK, np.array(new_sizes)


def mine(xyz, track_off, track_img, adj, adj_tri, K, R, t, image_sizes, *, nb_src, nb_per_scene, nb_points_thresh, usable, has_depth,
         rng, min_size=512):
    """The miner's loop on arrays.  -> (tuples, log): tuples a list of dict(idx_list, K, sizes, min_d, max_d); log counts what
    happened to candidates and tuples (rejected_adj, rejected_tri, dropped_depth, dropped_range, short)."""
    n = len(adj)
    log = dict(rejected_adj=0, rejected_tri=0, dropped_depth=0, dropped_range=0, short=0)
    found = []
    for ref in rng.permutation(n):
        if not usable[ref]:
            continue
        srcs = []
        for c in rng.permutation(n - 1):
            if c == ref or adj[ref, c] <= 0 or not usable[c]:
                continue
            if adj[ref, c] <= nb_points_thresh:
                log["rejected_adj"] += 1
                continue
            if adj_tri[ref, c] <= nb_points_thresh:
                log["rejected_tri"] += 1
                continue
            srcs.append(int(c))
            if len(srcs) >= nb_src:
                break
        if len(srcs) < nb_src:
            log["short"] += 1
        else:
            if not has_depth[ref]:
                log["dropped_depth"] += 1
                continue
            idx_list = [int(ref)] + srcs
            newK, new_sizes = rescaled(K, image_sizes, idx_list, min_size)
            min_d, max_d, _, _ = visible_range(xyz, track_off, track_img, idx_list, newK, R, t, new_sizes)
            if min_d is None:
                log["dropped_range"] += 1
                continue
            found.append(dict(idx_list=idx_list, K=newK, sizes=new_sizes, min_d=min_d, max_d=max_d))
        if len(found) >= nb_per_scene:
            break
    return found, log


# ---- synthetic scenes (arrays only) --------------------------------------------------------------------------------------------
def intrinsics(n, rng, width=640, height=480):
    K = np.zeros((n, 3, 3), dtype=np.float32)
    K[:, 0, 0], K[:, 1, 1] = rng.uniform(480, 560, n), rng.uniform(480, 560, n)
    K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = width / 2, height / 2, 1
    return K, np.tile(np.array([[width, height]], dtype=np.float64), (n, 1))


def scene(n_images, n_points, lengths, seed, spacing=0.3):
    """tests/_scene_setup_ref.py:synthetic_scene plus per-image intrinsics and sizes: dict(xyz, track_off, track_img, R, t, K, sizes)."""
    from tests import _scene_setup_ref as SR
    sc = SR.synthetic_scene(n_images, n_points, lengths, seed, spacing)
    sc["K"], sc["sizes"] = intrinsics(n_images, np.random.default_rng(seed + 1))
    return sc


def tuples_of(sc, tuples):
    """(tuples int32 [T,V], K fp32 [T,V,3,3], sizes fp64 [T,V,2]) of the scene's own cameras."""
    tuples = np.asarray(tuples, dtype=np.int32)
    return tuples, sc["K"][tuples], sc["sizes"][tuples]


def scene_70(T, V, seed=0):
    """70 images (the bitmask spans three words), 1003 points (no multiple of the block), tracks of 2..70 images; T tuples of V
    neighbouring image indices each, starting anywhere (so that they straddle the words)."""
    rng = np.random.default_rng(100 + seed)
    lengths = np.concatenate([[70, 70, 69, 66, 65, 64, 63], rng.integers(2, 40, 1003 - 7)])
    sc = scene(70, 1003, lengths, seed=70 + seed)
    starts = rng.integers(0, 70, T)
    starts[0] = 28                                                       # images 28..: around the boundary of words 0 and 1
    tuples = np.stack([rng.permutation((s + np.arange(2 * V)) % 70)[:V] for s in starts])
    return sc, tuples_of(sc, tuples)


def scene_edges():
    """The edge cases in one scene of 12 images and 73 points, every point seen by images 0..4 unless said otherwise; tuple 0 =
    images (0,1,2,3,4), tuple 1 = (5,6,7,8) of which no point has 3, tuple 2 = (0,1,2,9): image 9 stands 1000 to the side, so no point
    is valid in it.  Rows 0..5 are placed by hand relative to image 0: behind it, left / right / above / below its bounds, and far
    in front (valid, the farthest).  Rows 6, 7 are one point twice, nearer than all others, and rows 8, 9 repeat row 5 (equal depths:
    the lowest row wins); the rest is a cloud in front of the rig.  Row 72 is seen by two images only."""
    from tests import _scene_setup_ref as SR
    rng = np.random.default_rng(5)
    n = 12
    R, t = SR.rig(n, rng, 0.3)
    R64 = R.astype(np.float64)
    centre9 = -R64[9].T @ t[9].astype(np.float64) + np.array([1000.0, 0.0, 0.0])
    t[9] = (-R64[9] @ centre9).astype(np.float32)
    K, sizes = intrinsics(n, rng)
    c0 = -R64[0].T @ t[0].astype(np.float64)
    ray = lambda px, py, d: c0 + R64[0].T @ (np.linalg.inv(K[0].astype(np.float64)) @ np.array([px, py, 1.0]) * d)
    hand = [ray(320, 240, -4.0), ray(-900, 240, 5.0), ray(1500, 240, 5.0), ray(320, -700, 5.0), ray(320, 1200, 5.0), ray(320, 240, 30.0)]
    cloud = np.stack([rng.uniform(-0.8, 0.8, 63), rng.uniform(-0.6, 0.6, 63), rng.uniform(3, 7, 63)], axis=1)
    near = np.array([0.0, 0.0, 2.5])
    xyz = np.concatenate([np.array(hand), [near, near, hand[5], hand[5]], cloud])
    assert len(xyz) == 73
    tracks = [[0, 1, 2, 3, 4]] * 72 + [[0, 1]]
    tracks[20] = [0, 1, 2, 3, 4, 5, 6]                                   # two of tuple 1's images: not enough
    tracks[21] = [0, 2, 4, 9, 10]
    off = np.zeros(len(tracks) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(tr) for tr in tracks])
    img = np.array([i for tr in tracks for i in tr], dtype=np.int32)
    sc = dict(xyz=xyz, track_off=off, track_img=img, R=R, t=t, K=K, sizes=sizes)
    return sc, [tuples_of(sc, [[0, 1, 2, 3, 4]]), tuples_of(sc, [[5, 6, 7, 8]]), tuples_of(sc, [[0, 1, 2, 9]])]


def bench_scene(n_images=2000, n_points=300000, mean=8.0, seed=0):
    """A scene of MegaDepth proportions for scripts/bench_md_tuples.py: tests/_scene_setup_ref.py:bench_scene with intrinsics."""
    from tests import _scene_setup_ref as SR
    return scene(n_images, n_points, SR.heavy_tailed_lengths(n_points, mean, n_images, seed), seed)
