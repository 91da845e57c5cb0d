"""Scene set-up from a COLMAP sparse model, the part of the reference's ``utils/colmap_utils.py`` that every YFCC scene starts with
(``data/yfcc_scene.py:init_calibs``): calibration arrays, each image's source views and its depth range.  INTEGRATION.md
section 2i.

``compute_min_max_depth_visible`` is the depth range of an image tuple that the MegaDepth tuple mining needs (``preprocess.py``;
INTEGRATION.md section 2j), with a batched form over many tuples: ``ops.tuple_visible_depths``.

``compute_Kmatrix_colmap`` and ``get_calib_from_sparse`` are host code.  ``compute_src_imgs`` and ``compute_min_max_depth_yao``
flatten the model into index arrays on the host (once, O(observations)), upload them and run on the GPU:
``ops.sparse_pair_counts`` / ``ops.sparse_depth_ranges`` (csrc/scene_setup.hip).  There is no CPU path: without a HIP device the
ops raise.  The functions take the dicts of namedtuples of ``utils/colmap_model.py`` or of the reference's own model reader
(same field names), in the dict's order, which is the order of the rows of ``K``, ``R`` and ``t``."""
from __future__ import annotations

import numpy as np
import torch

from .. import ops


def compute_Kmatrix_colmap(params):
    """3 x 3 intrinsics of a PINHOLE camera's (fx, fy, cx, cy)."""
    return np.array([[params[0], 0, params[2]], [0, params[1], params[3]], [0, 0, 1]])


def _rotations_from_qvec(qvec):
    """[n,4] unit quaternions in COLMAP's order (w, x, y, z) -> [n,3,3] rotations: with scalar part w and vector part v,
    R = (w^2 - v.v) I + 2 v v^T + 2 w [v]_x, where [v]_x is the cross-product matrix of v."""
    qvec = np.asarray(qvec, dtype=np.float64).reshape(-1, 4)
    w, v = qvec[:, 0], qvec[:, 1:]
    cross = np.zeros((len(qvec), 3, 3))
    cross[:, 0, 1], cross[:, 0, 2], cross[:, 1, 2] = -v[:, 2], v[:, 1], -v[:, 0]
    cross -= cross.transpose(0, 2, 1)
    scale = w * w - np.einsum("ni,ni->n", v, v)
    return scale[:, None, None] * np.eye(3) + 2.0 * np.einsum("ni,nj->nij", v, v) + 2.0 * w[:, None, None] * cross


def get_calib_from_sparse(cameras, images):
    """(K fp32 [N,3,3], R fp32 [N,3,3], t fp32 [N,3,1], sizes fp32 [N,2] = (width, height)) in the order of ``images``."""
    cams = [cameras[images[idx].camera_id] for idx in images]
    K = np.array([compute_Kmatrix_colmap(c.params) for c in cams], dtype=np.float32)
    sizes = np.array([[c.width, c.height] for c in cams], dtype=np.float32).reshape(-1, 2)
    R = _rotations_from_qvec([images[idx].qvec for idx in images]).astype(np.float32)
    t = np.array([images[idx].tvec for idx in images], dtype=np.float32).reshape(-1, 3)[..., None]
    return K, R, t, sizes


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError("colmap_utils: source views and depth ranges are computed on the MI355X only "
                           "(there is no CPU / PyTorch fallback); no HIP device is available")
    return torch.device("cuda", torch.cuda.current_device())


def _pose(R, t, n, dev):
    R = torch.as_tensor(np.asarray(R.cpu() if hasattr(R, "cpu") else R), dtype=torch.float32).reshape(-1, 3, 3)
    t = torch.as_tensor(np.asarray(t.cpu() if hasattr(t, "cpu") else t), dtype=torch.float32).reshape(-1, 3)
    if R.shape[0] != n or t.shape[0] != n:
        raise ValueError(f"colmap_utils: {n} images but R {tuple(R.shape)} and t {tuple(t.shape)}")
    return R.contiguous().to(dev), t.contiguous().to(dev)


def _lookup(ids, sorted_keys, order, what):
    """Position in the dict's order of every id of ``ids`` (``sorted_keys`` = the dict's keys sorted, ``order`` = their positions);
    an unknown id raises KeyError, as the reference's dict lookup does."""
    pos = np.searchsorted(sorted_keys, ids)
    pos[pos >= len(sorted_keys)] = 0
    bad = sorted_keys[pos] != ids if len(sorted_keys) else np.ones(len(ids), dtype=bool)
    if bad.any():
        raise KeyError(f"{what} {int(np.asarray(ids)[bad][0])} is not in the model")
    return order[pos]


def _index(keys):
    keys = np.fromiter(keys, dtype=np.int64)
    order = np.argsort(keys, kind="stable")
    return keys[order], order


def flatten_tracks(images, points3d):
    """(xyz fp64 [P,3], track_off int64 [P+1], track_img int32 [nnz]): the tracks of ``points3d`` in CSR form over image INDICES
    (positions in ``images``), sorted and de-duplicated per point -- the inputs of ``ops.sparse_pair_counts``."""
    pts = list(points3d.values())
    xyz = np.array([p.xyz for p in pts], dtype=np.float64).reshape(-1, 3)
    lens = np.array([len(p.image_ids) for p in pts], dtype=np.int64)
    ids = np.concatenate([np.asarray(p.image_ids, dtype=np.int64) for p in pts]) if len(pts) else np.zeros(0, np.int64)
    img = _lookup(ids, *_index(images.keys()), "image id") if len(ids) else np.zeros(0, np.int64)
    n = max(len(images), 1)
    pair = np.unique(np.repeat(np.arange(len(pts), dtype=np.int64), lens) * n + img)     # sorted by point, then image; no duplicates
    off = np.zeros(len(pts) + 1, dtype=np.int64)
    np.cumsum(np.bincount(pair // n, minlength=len(pts)), out=off[1:])
    return xyz, off, (pair % n).astype(np.int32)


def flatten_observations(points3d, imgs):
    """(xyz fp64 [P,3], obs_img int32 [M], obs_pt int32 [M]): every keypoint of ``imgs`` with a 3-D point (id != -1), image by
    image, as (image index, row of xyz) -- the inputs of ``ops.sparse_depth_ranges``."""
    xyz = np.array([p.xyz for p in points3d.values()], dtype=np.float64).reshape(-1, 3)
    per = [np.asarray(im.point3D_ids, dtype=np.int64) for im in imgs.values()]
    per = [p[p != -1] for p in per]
    ids = np.concatenate(per) if per else np.zeros(0, np.int64)
    obs_img = np.repeat(np.arange(len(per), dtype=np.int32), [len(p) for p in per]) if per else np.zeros(0, np.int32)
    obs_pt = _lookup(ids, *_index(points3d.keys()), "point3D id") if len(ids) else np.zeros(0, np.int64)
    return xyz, obs_img.astype(np.int32), obs_pt.astype(np.int32)


def select_source_views(adj, adj_tri, nsrc):
    """The reference's choice from the two count matrices (device tensors) -> int64 [N, min(nsrc, N)] on the device: row i zeroes
    every ``adj[i,j]`` with ``adj_tri[i,j] < 0.75 adj[i,j]`` (4 adj_tri < 3 adj, exact in integers), sorts the row ascending with a
    stable sort and keeps the last ``nsrc`` indices in that order -- ``np.argsort(row)[-nsrc:]`` wherever that is deterministic."""
    a, tri = adj.to(torch.int64), adj_tri.to(torch.int64)
    common = torch.where(4 * tri < 3 * a, torch.zeros_like(a), a)
    return torch.sort(common, dim=1, stable=True).indices[:, -int(nsrc):]


def compute_src_imgs(images, points3d, R, t, min_triangulation_angle, nsrc, nb_points_thresh):
    """Each image's ``nsrc`` source views, a list of lists of image indices (ascending by shared points, best last), as the
    reference's function of the same name returns with ``nb_points_thresh=None``."""
    if nb_points_thresh is not None:
        raise NotImplementedError(
            "compute_src_imgs: nb_points_thresh is not supported.  The reference's branch takes len() of np.nonzero()'s TUPLE, "
            "which is 1, so it returns an empty list for every image whenever nsrc > 1, and otherwise draws at random: there is "
            "no defined answer to reproduce.  Pass nb_points_thresh=None.")
    if int(nsrc) < 1:
        raise ValueError(f"compute_src_imgs: nsrc={nsrc} < 1")
    dev = _device()
    xyz, off, img = flatten_tracks(images, points3d)
    Rd, td = _pose(R, t, len(images), dev)
    adj, adj_tri = ops.sparse_pair_counts(torch.from_numpy(xyz).to(dev), torch.from_numpy(off).to(dev), torch.from_numpy(img).to(dev),
                                          Rd, td, float(min_triangulation_angle))
    return select_source_views(adj, adj_tri, nsrc).cpu().tolist()


def compute_min_max_depth_yao(points3d, imgs, K, R, t, perc=(1, 99)):
    """(depth_min fp64 [N], depth_max fp64 [N], None, None): per image the ``perc`` percentiles of the depths of the 3-D points it
    observes (0, 0 for an image that observes none), as the reference's function of the same name.  ``K`` enters the reference's
    depth only through its last row, which must be (0, 0, 1)."""
    K = np.asarray(K.cpu() if hasattr(K, "cpu") else K).reshape(-1, 3, 3)
    if len(K) != len(imgs) or not np.array_equal(K[:, 2], np.broadcast_to(np.array([0, 0, 1], dtype=K.dtype), (len(K), 3))):
        raise ValueError("compute_min_max_depth_yao: K must be [N,3,3] with last rows (0, 0, 1)")
    dev = _device()
    xyz, obs_img, obs_pt = flatten_observations(points3d, imgs)
    Rd, td = _pose(R, t, len(imgs), dev)
    lo, hi = ops.sparse_depth_ranges(torch.from_numpy(xyz).to(dev), torch.from_numpy(obs_img).to(dev), torch.from_numpy(obs_pt).to(dev),
                                     Rd, td, perc)
    return lo.cpu().numpy(), hi.cpu().numpy(), None, None


def flatten_tracks_strict(images, points3d):
    """``flatten_tracks`` under the precondition of the tuple mining, checked: no track holds an image twice and no image's
    ``point3D_ids`` hold a point twice (COLMAP guarantees both); ValueError otherwise.  Only then is the count of shared points a
    set count, as the engine's ``adj``, and a multiset count, as the reference's script, at once."""
    xyz, off, img = flatten_tracks(images, points3d)
    lens = np.array([len(p.image_ids) for p in points3d.values()], dtype=np.int64)
    if not np.array_equal(np.diff(off), lens):
        bad = list(points3d)[int(np.nonzero(np.diff(off) != lens)[0][0])]
        raise ValueError(f"colmap_utils: the track of point {bad} holds an image more than once")
    for im_id, im in images.items():
        ids = np.asarray(im.point3D_ids, dtype=np.int64)
        ids = ids[ids != -1]
        if len(np.unique(ids)) != len(ids):
            raise ValueError(f"colmap_utils: image {im_id} observes a 3-D point more than once")
    return xyz, off, img


def tuple_visible_depths(flat, tuples, K, R, t, sizes):
    """The batched form of ``compute_min_max_depth_visible``: ``flat`` = (xyz, track_off, track_img) of ``flatten_tracks`` as numpy
    arrays or device tensors; tuples [T,V] image indices; K [T,V,3,3]; R [N,3,3], t [N,3(,1)] of all images; sizes [T,V,2] = (w, h)
    -> numpy (min_d fp64 [T,V], max_d fp64 [T,V], min_row int64 [T,V], max_row int64 [T,V], n_pts int32 [T]).  A tuple has a range
    when ``n_pts > 0`` and no ``min_row`` is -1."""
    dev = _device()
    put = lambda x, dt: (x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))).to(device=dev, dtype=dt).contiguous()
    xyz, off, img = put(flat[0], torch.float64), put(flat[1], torch.int64), put(flat[2], torch.int32)
    tuples = np.asarray(tuples)
    if tuples.ndim != 2:
        raise ValueError(f"colmap_utils: tuples [T,V] expected, got {tuples.shape}")
    T, V = tuples.shape
    Rd, td = _pose(R, t, len(np.asarray(R.cpu() if hasattr(R, "cpu") else R).reshape(-1, 3, 3)), dev)
    out = ops.tuple_visible_depths(xyz, off, img, put(tuples, torch.int32), put(np.asarray(K).reshape(T, V, 3, 3), torch.float32), Rd, td,
                                   put(np.asarray(sizes).reshape(T, V, 2), torch.float64))
    return tuple(o.cpu().numpy() for o in out)


def compute_min_max_depth_visible(points3d, imgs, K, R, t, sizes, *, images=None):
    """(min_d fp64 [V], max_d fp64 [V], min_point fp64 [V,3], max_point fp64 [V,3]) of the tuple of images ``imgs`` (COLMAP image
    ids; K [V,3,3], R [V,3,3], t [V,3,1], sizes [V,2] = (w, h) are the tuple's rows), as the reference's function of the same name:
    over the points that at least 3 of the tuple's images observe, per view the smallest and largest depth among those that
    project inside the image with a positive depth, and the points that attain them.  (None, None, None, None) when a view has no
    such point or no point has 3 observations.  (The reference returns the four None in the first case; in the second it fails
    with a ValueError of its reshape, outside its ``try``: that is answered with the four None as well.)

    ``images`` is not in the reference's signature: the model's image dict.  With it, ``imgs`` must be keys of it and the tracks
    are flattened over its key order, as everywhere in this module; without it, the tuple's ids alone are indexed and other ids
    in the tracks are ignored.  The result is the same; ``images`` checks the ids against the model."""
    imgs = [int(i) for i in imgs]
    V = len(imgs)
    if images is not None:
        keys = list(images.keys())
        missing = [i for i in imgs if i not in images]
        if missing:
            raise KeyError(f"image id {missing[0]} is not in the model")
    else:
        keys = imgs
    if len(set(imgs)) != V:
        raise ValueError("compute_min_max_depth_visible: an image id occurs twice in the tuple")
    sorted_keys, order = _index(keys)
    pts = list(points3d.values())
    xyz = np.array([p.xyz for p in pts], dtype=np.float64).reshape(-1, 3)
    lens = np.array([len(p.image_ids) for p in pts], dtype=np.int64)
    ids = np.concatenate([np.asarray(p.image_ids, dtype=np.int64) for p in pts]) if len(pts) else np.zeros(0, np.int64)
    pos = np.minimum(np.searchsorted(sorted_keys, ids), len(sorted_keys) - 1)
    known = sorted_keys[pos] == ids                                       # (ids outside ``keys``: no image of the tuple)
    n = len(keys)
    pair = np.unique(np.repeat(np.arange(len(pts), dtype=np.int64), lens)[known] * n + order[pos[known]])
    off = np.zeros(len(pts) + 1, dtype=np.int64)
    np.cumsum(np.bincount(pair // n, minlength=len(pts)), out=off[1:])
    idx = _lookup(np.array(imgs, dtype=np.int64), sorted_keys, order, "image id")
    as_np = lambda x: np.asarray(x.cpu() if hasattr(x, "cpu") else x)
    R_all = np.tile(np.eye(3, dtype=np.float32), (n, 1, 1))
    t_all = np.zeros((n, 3), dtype=np.float32)
    R_all[idx] = as_np(R).reshape(V, 3, 3)
    t_all[idx] = as_np(t).reshape(V, 3)
    min_d, max_d, min_row, max_row, n_pts = tuple_visible_depths((xyz, off, (pair % n).astype(np.int32)), idx[None], as_np(K).reshape(1, V, 3, 3),
                                                                 R_all, t_all, as_np(sizes).reshape(1, V, 2))
    if n_pts[0] == 0 or (min_row[0] < 0).any():
        return None, None, None, None
    return min_d[0], max_d[0], xyz[min_row[0]], xyz[max_row[0]]
