"""CPU: the MegaDepth tuple mining's host side.  The numpy restatement tests/_md_tuples_ref.py must
reproduce what the reference computed for tests/golden/md_tiny (md_tiny_expected.npz, written by gen_golden_md.py): the visible
ranges and points of the hand-picked tuples, the tuple without a range, and the mined tuple list; ``getResizedSize`` its recorded
values; ``select_tuple_candidates`` the recorded candidates from the fixture's matrices and permutations; ``save_infos`` the
reference's keys; and the new prototypes of include/pscv.h are bound."""
import functools
import os

import numpy as np
import pytest

from tests import _md_tuples_ref as MR
from tests import _scene_setup_ref as SR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@functools.lru_cache(maxsize=None)
def md_tiny():
    """(cameras, images, points, expected, flattened model, calibration): read once, never written to."""
    from wild_deep_mvs_amd.utils import colmap_model as CM
    from wild_deep_mvs_amd.utils import colmap_utils as CU
    d = os.path.join(GOLDEN, "md_tiny")
    cameras = CM.read_cameras_binary(os.path.join(d, "cameras.bin"))
    images, points = CM.read_images_binary(os.path.join(d, "images.bin")), CM.read_points3D_binary(os.path.join(d, "points3D.bin"))
    want = dict(np.load(os.path.join(GOLDEN, "md_tiny_expected.npz")))
    xyz, off, img, _, _ = SR.flatten_model(images, points)
    return cameras, images, points, want, (xyz, off, img), CU.get_calib_from_sparse(cameras, images)


def hand_tuples(want):
    for k in range(int(want["n_hand"])):
        yield k, {name: want[f"hand{k}_{name}"] for name in ("idx", "K", "sizes", "none")}


def test_the_fixture_covers_what_it_is_for():
    want = md_tiny()[3]
    assert int(want["nb_points_thresh"]) == 8 and float(want["triangulation_angle_threshold"]) == 5.0
    assert (want["log"][:4] > 0).all(), "a rejection by adj, one by adj_tri, a drop for the depth file and one for the range"
    assert sum(bool(h["none"]) for _, h in hand_tuples(want)) >= 1 and len(want["mined_idx"]) == int(want["nb_per_scene"])


def test_restatement_reproduces_the_references_ranges_and_points():
    _, _, _, want, (xyz, off, img), (K, R, t, _) = md_tiny()
    for k, h in hand_tuples(want):
        got = MR.visible_range(xyz, off, img, h["idx"], h["K"], R, t, h["sizes"])
        if h["none"]:
            assert got == (None, None, None, None), f"tuple {k}"
            continue
        for name, g in zip(("min_d", "max_d", "min_point", "max_point"), got):
            w = want[f"hand{k}_{name}"]
            assert g.dtype == np.float64 and g.shape == w.shape
            if name.endswith("point"):
                assert np.array_equal(g, w), f"tuple {k} {name}"
            else:
                assert np.allclose(g, w, rtol=1e-12, atol=0), f"tuple {k} {name}"


def test_restatement_mines_the_references_tuples():
    _, _, _, want, (xyz, off, img), (K, R, t, _) = md_tiny()
    adj, adj_tri, _ = SR.pair_counts(xyz, off, img, R, t, float(want["triangulation_angle_threshold"]))
    assert np.array_equal(adj, want["adj"]) and np.array_equal(adj_tri, want["adj_tri"])
    rng = np.random.RandomState(int(want["seed"]))
    mined, log = MR.mine(xyz, off, img, adj, adj_tri, K, R, t, want["image_sizes"], nb_src=int(want["nb_src"]),
                         nb_per_scene=int(want["nb_per_scene"]), nb_points_thresh=int(want["nb_points_thresh"]), usable=want["usable"],
                         has_depth=want["has_depth"], rng=rng, min_size=int(want["min_size"]))
    assert [m["idx_list"] for m in mined] == want["mined_idx"].tolist()
    assert [log[k] for k in ("rejected_adj", "rejected_tri", "dropped_depth", "dropped_range", "short")] == want["log"].tolist()
    assert rng.random_sample() == float(want["rng_after"]), "the generator is left where the script leaves it"
    for k, m in enumerate(mined):
        assert np.array_equal(m["K"], want["mined_K"][k]) and m["K"].dtype == np.float32
        assert np.array_equal(m["sizes"], want["mined_sizes"][k])
        assert np.allclose(m["min_d"], want["mined_min_d"][k], rtol=1e-12, atol=0)
        assert np.allclose(m["max_d"], want["mined_max_d"][k], rtol=1e-12, atol=0)


def test_get_resized_size_reproduces_the_recorded_values():
    from wild_deep_mvs_amd.preprocess import getResizedSize
    want = md_tiny()[3]
    for size, out in zip(want["resize_in"].tolist(), want["resize_out"].tolist()):
        assert list(getResizedSize(tuple(size), int(want["min_size"]))) == out
        assert list(MR.resized_size(tuple(size), int(want["min_size"]))) == out


def test_select_tuple_candidates_gives_the_recorded_candidates():
    from wild_deep_mvs_amd.preprocess import select_tuple_candidates
    want = md_tiny()[3]
    n_drawn = len(want["perms_src"])
    usable_seen = np.cumsum(want["usable"][want["perm_ref"]])
    perm_ref = want["perm_ref"][:int(np.searchsorted(usable_seen, n_drawn)) + 1]        # as far as the script walked
    got = select_tuple_candidates(want["adj"], want["adj_tri"], want["usable"], perm_ref, list(want["perms_src"]),
                                  nb_src=int(want["nb_src"]), nb_points_thresh=int(want["nb_points_thresh"]))
    assert [ref for ref, _ in got] == want["cand_ref"].tolist()
    assert [srcs if srcs is not None else [-1] * int(want["nb_src"]) for _, srcs in got] == want["cand_srcs"].tolist()
    with pytest.raises(ValueError, match="select_tuple_candidates"):
        select_tuple_candidates(want["adj"], want["adj_tri"], want["usable"], perm_ref, list(want["perms_src"])[:-1],
                                nb_src=int(want["nb_src"]), nb_points_thresh=int(want["nb_points_thresh"]))


def test_select_tuple_candidates_never_takes_the_reference_or_an_unshared_image():
    from wild_deep_mvs_amd.preprocess import select_tuple_candidates
    adj = np.array([[9, 5, 0, 7], [5, 9, 6, 0], [0, 6, 9, 0], [7, 0, 0, 9]])
    tri = np.array([[0, 5, 0, 7], [5, 0, 1, 0], [0, 1, 0, 0], [7, 0, 0, 0]])
    usable = np.array([True, True, True, False])
    got = select_tuple_candidates(adj, tri, usable, [0, 3, 1], [[0, 2, 1], [1, 2, 0]], nb_src=1, nb_points_thresh=-1)
    assert got == [(0, [1]), (1, [2])]        # 0 itself and the unshared 2 are passed over; the unusable 3 draws no permutation
    assert select_tuple_candidates(adj, tri, usable, [1], [[1, 2, 0]], nb_src=1, nb_points_thresh=1) == [(1, [0])]
    assert select_tuple_candidates(adj, tri, usable, [1], [[1, 2, 0]], nb_src=2, nb_points_thresh=1) == [(1, None)]


def test_save_infos_writes_the_references_keys(tmp_path):
    from wild_deep_mvs_amd.preprocess import save_infos
    tup = dict(ref=3, srcs=[1, 2], idx_list=[0, 1, 2], K=np.ones((3, 3, 3), np.float32), R=np.ones((3, 3, 3), np.float32),
               t=np.ones((3, 3, 1), np.float32), sizes=np.ones((3, 2), np.int64), min_d=np.arange(3.0), max_d=np.arange(3.0) + 1)
    path = save_infos(tmp_path, 7, tup)
    assert os.path.basename(path) == "infos_7.npz"
    got = np.load(path)
    assert sorted(got.files) == ["K", "R", "max_d", "min_d", "t"]
    assert all(np.array_equal(got[k], tup[k]) and got[k].dtype == tup[k].dtype for k in got.files)


def test_flatten_tracks_strict_raises_on_a_repeated_observation():
    from wild_deep_mvs_amd.utils import colmap_utils as CU
    _, images, points, _, (xyz, off, img), _ = md_tiny()
    got = CU.flatten_tracks_strict(images, points)
    assert np.array_equal(got[0], xyz) and np.array_equal(got[1], off) and np.array_equal(got[2], img)
    pid = next(iter(points))
    twice = dict(points)
    twice[pid] = points[pid]._replace(image_ids=np.concatenate([points[pid].image_ids, points[pid].image_ids[:1]]))
    with pytest.raises(ValueError, match=f"point {pid} holds an image more than once"):
        CU.flatten_tracks_strict(images, twice)
    iid = next(iter(images))
    seen = dict(images)
    seen[iid] = images[iid]._replace(point3D_ids=np.concatenate([images[iid].point3D_ids, images[iid].point3D_ids[:1]]))
    with pytest.raises(ValueError, match=f"image {iid} observes a 3-D point more than once"):
        CU.flatten_tracks_strict(seen, points)


def test_the_new_prototypes_are_bound():
    import ctypes as C
    from wild_deep_mvs_amd import _lib as L
    res, args = L.PROTOTYPES["pscv_tuple_visible_depths"]
    assert res is C.c_int and len(args) == 20 and args[3] is C.c_long and args[10] is C.c_int and args[-1] is C.c_void_p
    assert L.PROTOTYPES["pscv_tuple_visible_depths_workspace"] == (C.c_long, [C.c_int, C.c_int])
    assert L.ABI_VERSION == 14


def test_the_miner_has_no_cpu_path(monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    from wild_deep_mvs_amd.preprocess import mine_tuples
    cameras, images, points = md_tiny()[:3]
    with pytest.raises(RuntimeError, match="no CPU"):
        mine_tuples(cameras, images, points, nb_src=4, nb_per_scene=1)
