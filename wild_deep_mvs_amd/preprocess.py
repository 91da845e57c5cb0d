"""Mine MegaDepth training tuples from a scene's sparse model, the part of the reference's ``preprocess.py`` that decides WHICH
images form a tuple and what its cameras and depth range are.

Per scene: one ``ops.sparse_pair_counts`` launch gives, for every ordered pair of images, the points they share (``adj``) and
those past the triangulation-angle threshold (``adj_tri``); the host walks the script's random permutations over these two
matrices (``select_tuple_candidates``, a pure function); ``ops.tuple_visible_depths`` gives the visible depth range of the
candidate tuples, a chunk of reference images per launch, and the tuples are accepted in the script's order.

The script's control flow is kept as it stands, quirks included:
  * reference images run in ``rng.permutation(N)`` order; each usable one draws ``rng.permutation(N - 1)`` over the FIRST N - 1
    images, so the last image of the model is never a source;
  * a candidate is taken when it is usable, shares more than ``nb_points_thresh`` points with the reference and more than
    ``nb_points_thresh`` of them pass the angle test; the first ``nb_src`` taken form the tuple;
  * a tuple whose reference has no depth file, or whose visible range does not exist, is dropped without being counted;
  * the random numbers are drawn by the same calls in the same order, and the generator is left in the state the script leaves it
    in: with the same seed the tuples are the script's.
Precondition (checked, ValueError): no track holds an image twice and no image observes a point twice.

The images of a tuple are resampled on the GPU too: ``resize_tuple_images`` is the script's ``getResizedSize`` +
``Image.resize(size, resample=Image.LANCZOS)``, byte for byte (``ops.resize_lanczos_u8``).

Out of scope: decoding and encoding the JPEG files and copying the ``.h5`` depth files.  ``usable``, ``has_depth`` and
``image_sizes`` stand for what the script learns from the files.  There is no CPU path: without a HIP device ``mine_tuples`` and
``resize_tuple_images`` raise, like the functions of ``utils/colmap_utils.py``."""
from __future__ import annotations

import os

import numpy as np
import torch

from . import ops
from .utils import colmap_utils as CU

REF_CHUNK = 256          # usable reference images per tuple_visible_depths launch


def getResizedSize(size, minSize):
    """(width, height) of an image of ``size`` = (w, h) scaled so that its shorter side is ``minSize``, both cut down to multiples
    of 32; the reference's values."""
    w, h = size
    ratio = min(w / minSize, h / minSize)
    return int(w / ratio / 32) * 32, int(h / ratio / 32) * 32


def resize_tuple_images(images_u8, minSize=512):
    """The images of one tuple as the script saves them (``preprocess.py:157-163``): every decoded image (uint8 [H,W,3] on the GPU,
    sizes may differ) resized to ``getResizedSize((W, H), minSize)`` with PIL's Lanczos filter -> (the resized uint8 [h,w,3] GPU
    images, their (width, height) as int64 [V,2]: the ``sizes`` of a mined tuple, what ``mine_tuples`` derives from
    ``image_sizes``).  One or two launches per image on the current stream."""
    sizes = [getResizedSize((int(im.shape[1]), int(im.shape[0])), minSize) for im in images_u8]
    return [ops.resize_lanczos_u8(im, s) for im, s in zip(images_u8, sizes)], np.array(sizes, dtype=np.int64).reshape(-1, 2)


def select_tuple_candidates(adj, adj_tri, usable, perm_ref, perms_src, *, nb_src, nb_points_thresh):
    """The script's choice of source images from the two count matrices (numpy [N,N]): for every USABLE image of ``perm_ref``, in
    order, walk its permutation (``perms_src`` holds one per usable image of ``perm_ref``, in that order) and take candidate c when
    c is not the reference, is usable, ``adj[ref,c] > 0`` (it shares a point at all), ``adj[ref,c] > nb_points_thresh`` and
    ``adj_tri[ref,c] > nb_points_thresh``; stop at ``nb_src``.  -> a list of (ref, srcs) per usable image, ``srcs`` None where
    fewer than ``nb_src`` candidates were taken."""
    usable = np.asarray(usable, dtype=bool)
    refs = [int(r) for r in perm_ref if usable[r]]
    if len(refs) != len(perms_src):
        raise ValueError(f"select_tuple_candidates: {len(refs)} usable reference images but {len(perms_src)} permutations")
    out = []
    for ref, perm in zip(refs, perms_src):
        perm = np.asarray(perm, dtype=np.int64)
        a, tri = adj[ref, perm], adj_tri[ref, perm]
        take = perm[(perm != ref) & usable[perm] & (a > 0) & (a > nb_points_thresh) & (tri > nb_points_thresh)][:nb_src]
        out.append((ref, take.tolist() if len(take) >= nb_src else None))
    return out


def _rng_state(rng):
    """(np.random and a RandomState have get_state / set_state; a Generator keeps its state in its bit generator)"""
    return rng.get_state() if hasattr(rng, "get_state") else rng.bit_generator.state


def _rng_restore(rng, state):
    if hasattr(rng, "set_state"):
        rng.set_state(state)
    else:
        rng.bit_generator.state = state


def mine_tuples(cameras, images, points3d, *, nb_src, nb_per_scene, nb_points_thresh=100, triangulation_angle_threshold=5, usable=None,
                has_depth=None, image_sizes=None, rng=np.random, min_size=512):
    """The training tuples of one scene, a list of at most ``nb_per_scene`` dicts in the script's order:
      ref, srcs     COLMAP image ids;  idx_list  their positions in ``images`` (reference first)
      K             fp32 [V,3,3], rows 0 and 1 rescaled to the resized image as the script does;  R fp32 [V,3,3], t fp32 [V,3,1]
      sizes         int64 [V,2] the resized (width, height);  min_d, max_d  fp64 [V] the visible depth range per view
    ``usable[i]``: image i's file exists; ``has_depth[i]``: its depth file exists and is large enough (both default to all True);
    ``image_sizes`` [N,2] = (width, height) of the image files, by default the cameras' sizes; ``rng``: ``np.random`` or any object
    with ``permutation`` (a RandomState or a Generator), left in the state the script leaves it in."""
    n = len(images)
    nb_src = int(nb_src)
    if not 2 <= nb_src <= 31:
        raise ValueError(f"mine_tuples: nb_src={nb_src} outside [2,31] (a tuple of 3 to 32 views)")
    if n < 2:
        raise ValueError(f"mine_tuples: {n} images")
    dev = CU._device()
    K, R, t, sizes = CU.get_calib_from_sparse(cameras, images)
    usable = np.ones(n, dtype=bool) if usable is None else np.asarray(usable, dtype=bool).reshape(n)
    has_depth = np.ones(n, dtype=bool) if has_depth is None else np.asarray(has_depth, dtype=bool).reshape(n)
    image_sizes = (sizes if image_sizes is None else np.asarray(image_sizes)).reshape(n, 2)
    keys = list(images.keys())
    xyz, off, img = CU.flatten_tracks_strict(images, points3d)
    flat = tuple(torch.from_numpy(x).to(dev) for x in (xyz, off, img))
    Rd, td = CU._pose(R, t, n, dev)
    adj, adj_tri = (m.cpu().numpy() for m in ops.sparse_pair_counts(*flat, Rd, td, float(triangulation_angle_threshold)))
    # per image, once: the resized size and the float32 factors of K's first two rows
    old = [(int(w), int(h)) for w, h in image_sizes]
    new = np.array([getResizedSize(s, min_size) for s in old], dtype=np.int64).reshape(n, 2)
    scale = np.array([[rw / w, rh / h] for (rw, rh), (w, h) in zip(new.tolist(), old)], dtype=np.float64).astype(np.float32)

    found = []
    perm_ref = rng.permutation(n)
    pos = 0
    while pos < n and len(found) < nb_per_scene:
        # the next chunk of reference images: REF_CHUNK usable ones, each with its permutation drawn in the script's order
        state = _rng_state(rng)
        end, perms = pos, []
        while end < n and len(perms) < REF_CHUNK:
            if usable[perm_ref[end]]:
                perms.append(rng.permutation(n - 1))
            end += 1
        cand = select_tuple_candidates(adj, adj_tri, usable, perm_ref[pos:end], perms, nb_src=nb_src, nb_points_thresh=nb_points_thresh)
        lists = [[ref] + srcs for ref, srcs in cand if srcs is not None and has_depth[ref]]
        ranges = {}
        if lists:
            idx = np.array(lists, dtype=np.int64)
            Kt = K[idx].copy()
            Kt[:, :, 0, :] *= scale[idx, 0][..., None]
            Kt[:, :, 1, :] *= scale[idx, 1][..., None]
            min_d, max_d, min_row, _, n_pts = CU.tuple_visible_depths(flat, idx, Kt, Rd, td, new[idx])
            for k, lst in enumerate(lists):
                ok = n_pts[k] > 0 and (min_row[k] >= 0).all()
                ranges[lst[0]] = (Kt[k], min_d[k], max_d[k]) if ok else None
        drawn = 0                                              # permutations the script would have drawn when it stops
        for ref, srcs in cand:
            drawn += 1
            if srcs is None or ranges.get(ref) is None:
                continue
            lst = [ref] + srcs
            Kt, lo, hi = ranges[ref]
            found.append(dict(ref=keys[ref], srcs=[keys[c] for c in srcs], idx_list=lst, K=Kt, R=R[lst], t=t[lst], sizes=new[lst],
                              min_d=lo, max_d=hi))
            if len(found) >= nb_per_scene:
                break
        if len(found) >= nb_per_scene and drawn < len(perms):  # the script stopped inside the chunk: draw what it drew, no more
            _rng_restore(rng, state)
            for _ in range(drawn):
                rng.permutation(n - 1)
        pos = end
    return found


def save_infos(out_dir, k, tup):
    """Write tuple ``k``'s ``infos_{k}.npz`` with the reference's keys: min_d, max_d, K, R, t."""
    path = os.path.join(str(out_dir), f"infos_{k}.npz")
    np.savez(path, min_d=tup["min_d"], max_d=tup["max_d"], K=tup["K"], R=tup["R"], t=tup["t"])
    return path
