#!/usr/bin/env python3
"""Generate the fixture of the MegaDepth tuple mining: a sparse model of 14 images and 600 points
written with the reference's own COLMAP writer to tests/golden/md_tiny/{cameras,images,points3D}.bin, and what the reference makes
of it in tests/golden/md_tiny_expected.npz (arrays only): the tuples its ``preprocess.py`` would mine under ``np.random.seed(s)``
and the visible ranges and points of a list of hand-picked tuples, one of which has none.

The reference's loop sits under ``__main__`` among file reads and writes, so this script drives the reference's OWN functions --
``get_calib_from_sparse``, ``quat_to_rot``, ``relative_pose``, ``compute_triangulation_angle``, ``compute_min_max_depth_visible``,
``getResizedSize`` -- with that loop's control flow written here in our words; the image files are stood for by ``usable`` (the
file exists), ``has_depth`` (the depth file exists and is large enough) and the cameras' sizes (the size PIL would report).

The model: three PINHOLE cameras, one of them (of image position BAD) with its principal point far outside the image, so that no
point projects into that image: a tuple with it has no visible range.  Images on a jittered grid; tracks of 3..8 images near one
another, every observation once.

The reference's answer must not rest on chance, so a seed is accepted only if
  * angle margin: no angle of a tested pair lies within 1e-3 degrees of the threshold (float32 poses in the engine, float64
    quaternions here);
  * projection margin: no projection of a participating point is within 1e-6 px of an image bound, and no depth within 1e-9 of 0;
  * argmin margin: in every (tuple, view) the two smallest and the two largest valid depths differ by more than 1e-9 of their size;
  * coverage: a candidate rejected by the count of shared points, one rejected by the count past the angle, a tuple dropped for its
    depth file and one dropped for its range all occur, and the mining stops at nb_per_scene;
  * the restatement tests/_md_tuples_ref.py agrees with the reference on every tuple and on every pair the loop tested.
Runs ONLY where the reference tree is available.  Usage:  python tests/golden/gen_golden_md.py"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)
from gen_golden import import_reference  # noqa: E402

N_IMAGES, N_POINTS, NB_SRC, NB_PER_SCENE, THRESH, MIN_ANGLE, MIN_SIZE = 14, 600, 4, 5, 8, 5, 512
SPACING = 0.4
BAD = 5                                        # position of the image whose camera sees nothing inside its bounds
UNUSABLE = [11]                                # positions of the images "without a file"
NO_DEPTH = [2, 8]                              # positions of the images "without a depth file"
IMAGE_IDS = [12, 3, 31, 8, 5, 19, 2, 40, 27, 14, 9, 22, 51, 7]
HAND = [[0, 1, 4], [1, 0, 4, 2, 6], [6, 7, 10, 3, 2, 9, 13, 12, 1, 0], [4, BAD, 1, 0], [13, 12, 9]]      # positions; the fourth has no range
RESIZE_CASES = [(640, 480), (512, 384), (1600, 1067), (1067, 1600), (513, 700), (3000, 2000), (512, 512), (600, 511), (33, 4000)]


def make_model(rw, seed):
    from tests import _scene_setup_ref as SR
    rng = np.random.default_rng(seed)
    R, t = SR.rig(N_IMAGES, rng, SPACING)
    cameras = {1: rw.Camera(id=1, model="PINHOLE", width=640, height=480, params=np.array([520.0, 522.5, 320.0, 240.0])),
               4: rw.Camera(id=4, model="PINHOLE", width=512, height=384, params=np.array([410.0, 411.0, 255.5, 190.25])),
               9: rw.Camera(id=9, model="PINHOLE", width=640, height=480, params=np.array([520.0, 521.0, -4000.0, 240.0]))}
    centre = -np.einsum("nji,nj->ni", R.astype(np.float64), t.astype(np.float64))
    near = np.argsort(np.linalg.norm(centre[:, None] - centre[None], axis=-1), axis=1)         # each image's neighbours, itself first
    obs = {k: [] for k in range(N_IMAGES)}
    points = {}
    for n in range(N_POINTS):
        pid = 2000 + 3 * n
        length = int(rng.integers(3, 9))
        pool = near[int(rng.integers(0, N_IMAGES)), :min(N_IMAGES, length + 3)]
        track = rng.choice(pool, length, replace=False).tolist()
        idxs = []
        for k in track:
            idxs.append(len(obs[k]))
            obs[k].append(pid)
        xyz = np.array([rng.uniform(-2, 2), rng.uniform(-2, 2), rng.uniform(3, 7)])
        points[pid] = rw.Point3D(id=pid, xyz=xyz, rgb=rng.integers(0, 256, 3).astype(np.uint8), error=float(rng.random()),
                                 image_ids=np.array([IMAGE_IDS[k] for k in track]), point2D_idxs=np.array(idxs))
    quat = np.concatenate([np.ones((N_IMAGES, 1)), rng.normal(0, 0.03, (N_IMAGES, 3))], axis=1)
    quat /= np.linalg.norm(quat, axis=1, keepdims=True)
    images = {}
    for k in range(N_IMAGES):
        ids = np.array(obs[k] + [-1, -1], dtype=np.int64)
        Rk = rw.qvec2rotmat(quat[k])
        images[IMAGE_IDS[k]] = rw.Image(id=IMAGE_IDS[k], qvec=quat[k], tvec=-Rk @ centre[k], camera_id=9 if k == BAD else (1 if k % 3 else 4),
                                        name=f"{k:08d}.jpg", xys=rng.random((len(ids), 2)) * 300, point3D_ids=ids)
    return cameras, images, points


def rescale(resized_size, K, image_sizes, idx_list):
    """The tuple's intrinsics and sizes after the resize: rows 0 and 1 of the float32 K times new / old width and height."""
    newK = K[idx_list].copy()
    new_sizes = []
    for k, i in enumerate(idx_list):
        w, h = image_sizes[i]
        rw_, rh_ = resized_size((w, h), minSize=MIN_SIZE)
        new_sizes.append((rw_, rh_))
        newK[k][0:1] *= rw_ / w
        newK[k][1:2] *= rh_ / h
    return newK, np.array(new_sizes)


def margins(U, points, ids, K, R, t, sizes):
    """(projection margin, depth margin, argmin margin) of one tuple from the reference's own projection."""
    pts = np.array([p.xyz for p in points.values() if sum(i in p.image_ids for i in ids) >= 3])
    if len(pts) == 0:
        return np.inf, np.inf, np.inf
    proj, depth = U.project_all(pts, K, R, t)
    bound = np.stack([np.abs(proj[..., 0]), np.abs(proj[..., 1]), np.abs(proj[..., 0] - sizes[:, 0, None]), np.abs(proj[..., 1] - sizes[:, 1, None])])
    valid = (np.all(proj >= 0, axis=2) & (proj[..., 0] < sizes[:, 0, None]) & (proj[..., 1] < sizes[:, 1, None]) & (depth > 0))
    arg = np.inf
    for v in range(len(ids)):
        d = np.sort(depth[v][valid[v]])
        if len(d) >= 2:
            arg = min(arg, (d[1] - d[0]) / abs(d[1]), (d[-1] - d[-2]) / abs(d[-1]))
    return float(bound.min()), float(np.abs(depth).min()), float(arg)


def drive(ref, U, resized_size, cameras, images, points, seed, usable, has_depth, image_sizes):
    """The reference's loop in our words.  -> dict of what it mined and what happened on the way."""
    np.random.seed(seed)
    K, R, t, _ = ref.get_calib_from_sparse(cameras, images)
    keys = list(images.keys())
    n = len(keys)
    out = dict(perm_ref=None, perms_src=[], cand_ref=[], cand_srcs=[], mined=[], none_tuples=[], pairs=[], angle_margin=np.inf,
               log=dict(rejected_adj=0, rejected_tri=0, dropped_depth=0, dropped_range=0, short=0))
    out["perm_ref"] = np.random.permutation(n)
    for idx in out["perm_ref"]:
        ref_id = keys[idx]
        if not usable[idx]:
            continue
        shared = {}
        for p in images[ref_id].point3D_ids:
            if p != -1:
                for other in points[p].image_ids:
                    if other != ref_id:
                        shared[other] = shared.get(other, 0) + 1
        perm = np.random.permutation(n - 1)
        out["perms_src"].append(perm)
        R1, t1 = U.quat_to_rot(images[ref_id].qvec[None]).squeeze(0), images[ref_id].tvec
        srcs, src_idx = [], []
        for j in perm:
            cid = keys[j]
            if cid not in shared or not usable[j]:
                continue
            if shared[cid] <= THRESH:
                out["log"]["rejected_adj"] += 1
                out["pairs"].append((int(idx), int(j), shared[cid], -1))
                continue
            R2, t2 = U.quat_to_rot(images[cid].qvec[None]).squeeze(0), images[cid].tvec
            common = set(images[ref_id].point3D_ids).intersection(images[cid].point3D_ids)
            cloud = np.array([points[p].xyz for p in common if p != -1])
            angle = U.compute_triangulation_angle(cloud, *U.relative_pose(R1, t1, R2, t2))
            out["angle_margin"] = min(out["angle_margin"], float(np.abs(angle - MIN_ANGLE).min()))
            past = int((angle > MIN_ANGLE).sum())
            out["pairs"].append((int(idx), int(j), shared[cid], past))
            if past <= THRESH:
                out["log"]["rejected_tri"] += 1
                continue
            srcs.append(cid)
            src_idx.append(int(j))
            if len(srcs) >= NB_SRC:
                break
        out["cand_ref"].append(int(idx))
        out["cand_srcs"].append(src_idx if len(srcs) >= NB_SRC else [-1] * NB_SRC)
        if len(srcs) >= NB_SRC:
            if not has_depth[idx]:
                out["log"]["dropped_depth"] += 1
                continue
            ids, idx_list = [ref_id] + srcs, [int(idx)] + src_idx
            newK, new_sizes = rescale(resized_size, K, image_sizes, idx_list)
            min_d, max_d, _, _ = ref.compute_min_max_depth_visible(points, ids, newK, R[idx_list], t[idx_list], new_sizes)
            if min_d is None or np.isnan(min_d).any() or np.isnan(max_d).any():
                out["log"]["dropped_range"] += 1
                out["none_tuples"].append(idx_list)
                continue
            out["mined"].append(dict(idx_list=idx_list, K=newK, sizes=new_sizes, min_d=min_d, max_d=max_d))
        else:
            out["log"]["short"] += 1
        if len(out["mined"]) >= NB_PER_SCENE:
            break
    out["rng_after"] = float(np.random.random())
    return out


def save_npz(path, arrays):
    """np.savez_compressed with a fixed time stamp on every member, so that the file regenerates bit for bit."""
    import io
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, buf.getvalue())


def main():
    import_reference()
    import utils.read_write_model_colmap as rw
    import utils.colmap_utils as ref
    import utils.utils_3D as U
    try:
        import preprocess as ref_pre
        resized_size = ref_pre.getResizedSize
    except Exception as e:                                        # (the script imports what this machine may lack)
        print(f"the reference's preprocess.py does not import here ({e!r}): getResizedSize restated")
        from tests._md_tuples_ref import resized_size as _rs
        resized_size = lambda size, minSize: _rs(size, minSize)
    from tests import _md_tuples_ref as MR
    from tests import _scene_setup_ref as SR
    np.int, np.bool = int, bool
    out_dir = os.path.join(HERE, "md_tiny")
    os.makedirs(out_dir, exist_ok=True)
    usable = np.ones(N_IMAGES, dtype=bool)
    usable[UNUSABLE] = False
    has_depth = np.ones(N_IMAGES, dtype=bool)
    has_depth[NO_DEPTH] = False

    def evaluate(cameras, images, points, seed):
        K, R, t, sizes = ref.get_calib_from_sparse(cameras, images)
        image_sizes = [(int(w), int(h)) for w, h in sizes]
        keys = list(images.keys())
        got = drive(ref, U, resized_size, cameras, images, points, seed, usable, has_depth, image_sizes)
        xyz, off, img, _, _ = SR.flatten_model(images, points)
        adj, adj_tri, _ = SR.pair_counts(xyz, off, img, R, t, MIN_ANGLE)
        pairs_ok = all(adj[i, j] == a and (tri < 0 or adj_tri[i, j] == tri) for i, j, a, tri in got["pairs"])
        hand = []
        for idx_list in HAND + got["none_tuples"]:
            newK, new_sizes = rescale(resized_size, K, image_sizes, idx_list)
            res = ref.compute_min_max_depth_visible(points, [keys[i] for i in idx_list], newK, R[idx_list], t[idx_list], new_sizes)
            hand.append(dict(idx_list=idx_list, K=newK, sizes=new_sizes, res=res))
        marg = [margins(U, points, [keys[i] for i in h["idx_list"]], h["K"], R[h["idx_list"]], t[h["idx_list"]], h["sizes"])
                for h in hand + got["mined"]]
        return got, hand, marg, pairs_ok, (xyz, off, img, adj, adj_tri, K, R, t, image_sizes)

    for seed in range(20261018, 20261018 + 400):
        cameras, images, points = make_model(rw, seed)
        got, hand, marg, pairs_ok, _ = evaluate(cameras, images, points, seed)
        log = got["log"]
        covered = all(log[k] > 0 for k in ("rejected_adj", "rejected_tri", "dropped_depth", "dropped_range")) and len(got["mined"]) == NB_PER_SCENE
        nones = [h["res"][0] is None for h in hand[:len(HAND)]]
        safe = (got["angle_margin"] > 1e-3 and min(m[0] for m in marg) > 1e-6 and min(m[1] for m in marg) > 1e-9
                and min(m[2] for m in marg) > 1e-9)
        if covered and safe and pairs_ok and nones == [False, False, False, True, False]:
            print(f"seed {seed}: {log}, angle margin {got['angle_margin']:.3e} deg, projection / depth / argmin margins "
                  f"{min(m[0] for m in marg):.3e} {min(m[1] for m in marg):.3e} {min(m[2] for m in marg):.3e}")
            break
    else:
        raise SystemExit("no seed met the conditions")
    rw.write_model(cameras, images, points, out_dir, ext=".bin")
    cameras, images, points = rw.read_model(out_dir, ext=".bin")                 # what the tests will read
    again, hand, marg, pairs_ok, (xyz, off, img, adj, adj_tri, K, R, t, image_sizes) = evaluate(cameras, images, points, seed)
    assert pairs_ok and again["log"] == got["log"] and again["rng_after"] == got["rng_after"]
    assert [m["idx_list"] for m in again["mined"]] == [m["idx_list"] for m in got["mined"]]
    # the restatement against the reference: every tuple, and the whole mining
    for h in hand:
        mine = MR.visible_range(xyz, off, img, h["idx_list"], h["K"], R, t, h["sizes"])
        if h["res"][0] is None:
            assert mine[0] is None
        else:
            for a, b in zip(h["res"], mine):
                assert np.allclose(a, b, rtol=1e-12, atol=0), "the restatement disagrees with the reference"
            assert np.array_equal(h["res"][2], mine[2]) and np.array_equal(h["res"][3], mine[3])
    mined, log = MR.mine(xyz, off, img, adj, adj_tri, K, R, t, image_sizes, nb_src=NB_SRC, nb_per_scene=NB_PER_SCENE, nb_points_thresh=THRESH,
                         usable=usable, has_depth=has_depth, rng=np.random.RandomState(seed), min_size=MIN_SIZE)
    assert log == again["log"] and [m["idx_list"] for m in mined] == [m["idx_list"] for m in again["mined"]]
    for a, b in zip(mined, again["mined"]):
        assert np.array_equal(a["K"], b["K"]) and np.array_equal(a["sizes"], b["sizes"])
        assert np.allclose(a["min_d"], b["min_d"], rtol=1e-12, atol=0) and np.allclose(a["max_d"], b["max_d"], rtol=1e-12, atol=0)
    keys = list(images.keys())
    arrays = dict(seed=np.int64(seed), nb_src=np.int64(NB_SRC), nb_per_scene=np.int64(NB_PER_SCENE), nb_points_thresh=np.int64(THRESH),
                  triangulation_angle_threshold=np.float64(MIN_ANGLE), min_size=np.int64(MIN_SIZE), usable=usable, has_depth=has_depth,
                  image_sizes=np.array(image_sizes, dtype=np.int64), bad_image=np.int64(BAD), rng_after=np.float64(again["rng_after"]),
                  adj=adj, adj_tri=adj_tri, perm_ref=np.asarray(again["perm_ref"], dtype=np.int64),
                  perms_src=np.array(again["perms_src"], dtype=np.int64), cand_ref=np.array(again["cand_ref"], dtype=np.int64),
                  cand_srcs=np.array(again["cand_srcs"], dtype=np.int64),
                  log=np.array([again["log"][k] for k in ("rejected_adj", "rejected_tri", "dropped_depth", "dropped_range", "short")], dtype=np.int64),
                  mined_idx=np.array([m["idx_list"] for m in again["mined"]], dtype=np.int64),
                  mined_ids=np.array([[keys[i] for i in m["idx_list"]] for m in again["mined"]], dtype=np.int64),
                  mined_K=np.array([m["K"] for m in again["mined"]]), mined_sizes=np.array([m["sizes"] for m in again["mined"]], dtype=np.int64),
                  mined_min_d=np.array([m["min_d"] for m in again["mined"]]), mined_max_d=np.array([m["max_d"] for m in again["mined"]]),
                  resize_in=np.array(RESIZE_CASES, dtype=np.int64),
                  resize_out=np.array([resized_size(s, minSize=MIN_SIZE) for s in RESIZE_CASES], dtype=np.int64),
                  n_hand=np.int64(len(hand)))
    for k, h in enumerate(hand):
        arrays[f"hand{k}_idx"] = np.array(h["idx_list"], dtype=np.int64)
        arrays[f"hand{k}_K"], arrays[f"hand{k}_sizes"] = h["K"], np.asarray(h["sizes"], dtype=np.int64)
        arrays[f"hand{k}_none"] = np.bool_(h["res"][0] is None)
        if h["res"][0] is not None:
            for name, a in zip(("min_d", "max_d", "min_point", "max_point"), h["res"]):
                arrays[f"hand{k}_{name}"] = np.asarray(a, dtype=np.float64)
    path = os.path.join(HERE, "md_tiny_expected.npz")
    save_npz(path, arrays)
    print(f"wrote {out_dir} and {path}: mined {[m['idx_list'] for m in again['mined']]}, tuples without a range {again['none_tuples']}")


if __name__ == "__main__":
    main()
