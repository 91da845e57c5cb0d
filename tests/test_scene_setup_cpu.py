"""CPU: scene set-up from a COLMAP sparse model.  The fixture tests/golden/scene_tiny (12 images, 300
points, written and answered by the reference: tests/golden/gen_golden_scene.py) against the numpy restatement of
tests/_scene_setup_ref.py, the model reader and the host functions of ``utils/colmap_utils.py``, and the refusal of
``nb_points_thresh``.  The GPU side is tests/test_gpu_scene_setup.py."""
import functools
import os

import numpy as np
import pytest

from tests import _scene_setup_ref as SR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@functools.lru_cache(maxsize=None)
def tiny():
    from wild_deep_mvs_amd.utils import colmap_model as CM
    d = os.path.join(GOLDEN, "scene_tiny")
    want = dict(np.load(os.path.join(GOLDEN, "scene_tiny.npz")))
    return CM.read_cameras_binary(os.path.join(d, "cameras.bin")), CM.read_images_binary(os.path.join(d, "images.bin")), \
        CM.read_points3D_binary(os.path.join(d, "points3D.bin")), want


def test_the_fixture_is_the_model_the_issue_asks_for():
    cameras, images, points, want = tiny()
    assert len(images) == 12 and len(points) == 300 and len(cameras) == 2
    lengths = [len(p.image_ids) for p in points.values()]
    assert min(lengths) == 2 and max(lengths) == 9
    assert sum(len(set(p.image_ids.tolist())) < len(p.image_ids) for p in points.values()) == 1      # one track names an image twice
    n_obs = [int((im.point3D_ids != -1).sum()) for im in images.values()]
    empty = int(want["empty_image"])
    assert n_obs[empty] == 0 and len(list(images.values())[empty].point3D_ids) > 0 and min(n for k, n in enumerate(n_obs) if k != empty) >= 20


def test_the_restatement_reproduces_the_reference():
    _, images, points, want = tiny()
    got = SR.scene_setup(images, points, want["R"], want["t"], min_triangulation_angle=float(want["min_triangulation_angle"]),
                         nsrc=int(want["nsrc"]))
    assert got["sel_idx"] == want["sel_idx"].tolist()
    np.testing.assert_allclose(got["depth_min"], want["depth_min"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(got["depth_max"], want["depth_max"], rtol=1e-12, atol=0)
    empty = int(want["empty_image"])
    assert got["depth_min"][empty] == 0 and got["depth_max"][empty] == 0 and not got["adj"][empty].any() and not got["adj"][:, empty].any()
    # what makes the answer well defined (the generator's conditions) and what makes it a test of the angle rule
    assert got["margin"] > 1e-3
    adj, tri = got["adj"], got["adj_tri"]
    assert np.array_equal(adj, adj.T) and not np.array_equal(tri, tri.T), "adj is symmetric, the reference's angle is not"
    assert not np.diag(tri).any() and np.array_equal(np.diag(adj), np.bincount(SR.flatten_model(images, points)[2], minlength=12))
    off = ~np.eye(12, dtype=bool) & (adj > 0)
    assert (4 * tri[off] < 3 * adj[off]).sum() >= 12 and (4 * tri[off] >= 3 * adj[off]).sum() >= 12, "some pairs pass the 75 % rule, some fail"
    common = np.where(4 * tri < 3 * adj, 0, adj)
    top = np.sort(np.delete(common, empty, axis=0), axis=1)[:, -(int(want["nsrc"]) + 1):]
    assert (top[:, 0] > 0).all() and (np.diff(top, axis=1) > 0).all(), "no choice rests on a tie"


def test_the_model_reader_and_the_calibration_reproduce_the_reference():
    from wild_deep_mvs_amd.utils import colmap_utils as CU
    cameras, images, _, want = tiny()
    assert {c.model for c in cameras.values()} == {"PINHOLE"} and sorted(cameras) == [1, 4]
    assert cameras[1].width == 640 and cameras[4].height == 384 and cameras[4].params.tolist() == [410.0, 411.0, 255.5, 190.25]
    K, R, t, sizes = CU.get_calib_from_sparse(cameras, images)
    for name, got in (("K", K), ("R", R), ("t", t), ("sizes", sizes)):
        assert got.dtype == np.float32 and got.shape == want[name].shape, name
        assert np.array_equal(got, want[name]), name
    assert t.shape == (12, 3, 1) and sizes[0].tolist() == [512.0, 384.0]
    assert np.array_equal(CU.compute_Kmatrix_colmap([2.0, 3.0, 4.0, 5.0]), [[2, 0, 4], [0, 3, 5], [0, 0, 1]])


def test_the_flattened_model_is_what_the_restatement_flattens():
    from wild_deep_mvs_amd.utils import colmap_utils as CU
    _, images, points, _ = tiny()
    xyz, off, img, obs_img, obs_pt = SR.flatten_model(images, points)
    x1, off1, img1 = CU.flatten_tracks(images, points)
    x2, oi, op = CU.flatten_observations(points, images)
    assert np.array_equal(x1, xyz) and np.array_equal(x2, xyz) and x1.dtype == np.float64
    assert np.array_equal(off1, off) and np.array_equal(img1, img) and off1.dtype == np.int64 and img1.dtype == np.int32
    assert np.array_equal(oi, obs_img) and np.array_equal(op, obs_pt) and oi.dtype == np.int32 and op.dtype == np.int32
    assert len(img) == sum(len(p.image_ids) for p in points.values()) - 1            # the doubled image counts once in its track
    assert len(oi) == sum(len(p.image_ids) for p in points.values())                 # ... and twice among its image's observations
    with pytest.raises(KeyError, match="image id"):
        CU.flatten_tracks({k: v for k, v in images.items() if k != 12}, points)


def test_nb_points_thresh_is_refused_with_the_reason():
    from wild_deep_mvs_amd.utils import colmap_utils as CU
    _, images, points, want = tiny()
    with pytest.raises(NotImplementedError, match="np.nonzero"):
        CU.compute_src_imgs(images, points, want["R"], want["t"], 5.0, 4, 10)


def test_select_source_views_is_the_restatements_choice_also_on_ties():
    import torch
    from wild_deep_mvs_amd.utils import colmap_utils as CU
    rng = np.random.default_rng(3)
    adj = rng.integers(0, 4, (9, 9))                                                 # small range: many ties, many zeros
    tri = np.minimum(adj, rng.integers(0, 4, (9, 9)))
    for nsrc in (1, 4, 9, 12):
        got = CU.select_source_views(torch.from_numpy(adj).to(torch.int32), torch.from_numpy(tri).to(torch.int32), nsrc).tolist()
        assert got == SR.select(adj, tri, nsrc)
