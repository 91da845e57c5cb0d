"""GPU: the MegaDepth tuple mining (csrc/scene_setup.hip:pscv_tuple_visible_depths behind ops.tuple_visible_depths,
utils/colmap_utils.py:compute_min_max_depth_visible and preprocess.py:mine_tuples).

Rows and point counts are integers and must EQUAL the numpy restatement's (tests/_md_tuples_ref.py) and the reference's
(tests/golden/md_tiny_expected.npz).  Depths: both sides are float64 on identical inputs and differ in summation order at most,
about 7 ulp of M = sum_k |K_3. R_.k x_k| + |K_3. t| + 1e-6 (three products and three sums in y_z = R_3. x + t_z, the same again in
u_z = K_3. y, one more sum for the 1e-6); the bar is 1e-14 M, a bit over ten times that.  Also the smallest shapes at which the
kernel can still go wrong, bit-reproducibility, and the argument errors."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import _md_tuples_ref as MR
from tests import _scene_setup_ref as SR

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BAR = 1e-14


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from wild_deep_mvs_amd import _lib as L, ops
    from wild_deep_mvs_amd.utils import colmap_utils as CU
    L.lib()
    return L, ops, CU


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


def _d(a, dt):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dt).cuda()


def _model(sc):
    return (_d(sc["xyz"], torch.float64), _d(sc["track_off"], torch.int64), _d(sc["track_img"], torch.int32),
            _d(sc["R"], torch.float32), _d(np.asarray(sc["t"]).reshape(-1, 3), torch.float32))


def _run(ops, sc, tuples, K, sizes):
    xyz, off, img, R, t = _model(sc)
    out = ops.tuple_visible_depths(xyz, off, img, _d(tuples, torch.int32), _d(K, torch.float32), R, t, _d(sizes, torch.float64))
    T, V = np.asarray(tuples).shape
    assert [o.dtype for o in out] == [torch.float64, torch.float64, torch.int64, torch.int64, torch.int32]
    assert all(o.is_cuda for o in out) and [tuple(o.shape) for o in out] == [(T, V)] * 4 + [(T,)]
    return [o.cpu().numpy() for o in out]


def _check(got, want, name):
    """Rows and counts equal; depths within the bar, printed before they are judged."""
    min_d, max_d, min_row, max_row, n_pts = got
    assert np.array_equal(n_pts, want["n_pts"]), f"{name}: n_pts gpu {n_pts.tolist()} restatement {want['n_pts'].tolist()}"
    assert np.array_equal(min_row, want["min_row"]), f"{name}: min_row gpu {min_row.tolist()} restatement {want['min_row'].tolist()}"
    assert np.array_equal(max_row, want["max_row"]), f"{name}: max_row gpu {max_row.tolist()} restatement {want['max_row'].tolist()}"
    none = want["min_row"] < 0
    assert np.isnan(min_d[none]).all() and np.isnan(max_d[none]).all() and (max_row[none] == -1).all()
    err_lo = np.abs(min_d - want["min_d"])[~none] / want["M_min"][~none]
    err_hi = np.abs(max_d - want["max_d"])[~none] / want["M_max"][~none]
    worst = max(err_lo.max(initial=0.0), err_hi.max(initial=0.0))
    print(f"{name}: worst depth error {worst:.3e} M (bar {BAR:.0e})")
    assert worst <= BAR, f"{name}: depth error {worst:.3e} M"


def _hand(want):
    for k in range(int(want["n_hand"])):
        yield k, {name: want[f"hand{k}_{name}"] for name in ("idx", "K", "sizes", "none")}


def test_op_equals_the_restatement_on_the_fixtures_tuples(env):
    _, ops, _ = env
    _, _, _, want, (xyz, off, img), (K, R, t, _) = md_tiny()
    sc = dict(xyz=xyz, track_off=off, track_img=img, R=R, t=t)
    by_v = {}
    for k, h in _hand(want):
        by_v.setdefault(len(h["idx"]), []).append(h)
    by_v.setdefault(want["mined_idx"].shape[1], []).extend(
        dict(idx=want["mined_idx"][k], K=want["mined_K"][k], sizes=want["mined_sizes"][k]) for k in range(len(want["mined_idx"])))
    for V, hs in sorted(by_v.items()):
        tuples, Kt, st = np.stack([h["idx"] for h in hs]), np.stack([h["K"] for h in hs]), np.stack([h["sizes"] for h in hs])
        _check(_run(ops, sc, tuples, Kt, st), MR.visible_depths_batch(xyz, off, img, tuples, Kt, R, t, st), f"md_tiny V={V} T={len(hs)}")


@pytest.mark.parametrize("T,V", [(7, 5), (3, 10)])
def test_op_on_70_images_and_1003_points(env, T, V):
    _, ops, _ = env
    sc, (tuples, K, sizes) = MR.scene_70(T, V)
    assert np.diff(sc["track_off"]).max() > 64 and len(sc["xyz"]) == 1003 and {int(i) // 32 for i in tuples[0]} == {0, 1}
    want = MR.visible_depths_batch(sc["xyz"], sc["track_off"], sc["track_img"], tuples, K, sc["R"], sc["t"], sizes)
    assert (want["n_pts"] > 0).all()
    _check(_run(ops, sc, tuples, K, sizes), want, f"scene_70 T={T} V={V}")


def test_op_edge_cases(env):
    """Behind a camera, outside each of the four bounds, duplicated points (the lowest row wins), a view without a valid point, a
    tuple without a 3-view point."""
    _, ops, _ = env
    sc, cases = MR.scene_edges()
    for k, (tuples, K, sizes) in enumerate(cases):
        want = MR.visible_depths_batch(sc["xyz"], sc["track_off"], sc["track_img"], tuples, K, sc["R"], sc["t"], sizes)
        if k == 0:                                            # what the scene was built for, on the restatement's side
            assert want["n_pts"][0] == 72
            assert (want["min_row"][0] == 6).all() and (want["max_row"][0] == 5).all(), "of the equal depths the lowest row"
            valid0 = MR.visible_depths_batch(sc["xyz"][:5], np.arange(6) * 3, np.tile([0, 1, 2], 5).astype(np.int32), [[0, 1, 2]], K[:, :3],
                                             sc["R"], sc["t"], sizes[:, :3])
            assert valid0["n_pts"][0] == 5 and valid0["min_row"][0, 0] == -1, "rows 0..4 are invalid in image 0, each for its own reason"
        if k == 1:
            assert want["n_pts"][0] == 0 and (want["min_row"] == -1).all()
        if k == 2:
            assert want["n_pts"][0] > 0 and want["min_row"][0, 3] == -1 and (want["min_row"][0, :3] >= 0).all()
        _check(_run(ops, sc, tuples, K, sizes), want, f"edges {k}")


def test_op_single_point_single_tuple(env):
    _, ops, _ = env
    sc, _ = MR.scene_edges()
    one = dict(sc, xyz=sc["xyz"][10:11], track_off=np.array([0, 3], dtype=np.int64), track_img=np.array([0, 1, 2], dtype=np.int32))
    tuples, K, sizes = MR.tuples_of(sc, [[2, 0, 1]])
    want = MR.visible_depths_batch(one["xyz"], one["track_off"], one["track_img"], tuples, K, sc["R"], sc["t"], sizes)
    assert want["n_pts"][0] == 1 and (want["min_row"] == 0).all() and (want["max_row"] == 0).all()
    _check(_run(ops, one, tuples, K, sizes), want, "T=1 V=3 P=1")
    none = dict(one, xyz=np.zeros((0, 3)), track_off=np.zeros(1, dtype=np.int64), track_img=np.zeros(0, dtype=np.int32))
    got = _run(ops, none, tuples, K, sizes)
    assert got[4][0] == 0 and (got[2] == -1).all() and (got[3] == -1).all() and np.isnan(got[0]).all() and np.isnan(got[1]).all()


def test_mirror_returns_the_references_arrays(env):
    _, _, CU = env
    _, images, points, want, _, (K, R, t, _) = md_tiny()
    keys = list(images.keys())
    for k, h in _hand(want):
        idx = h["idx"].tolist()
        ids = [keys[i] for i in idx]
        for kw in (dict(images=images), dict()):
            got = CU.compute_min_max_depth_visible(points, ids, h["K"], R[idx], t[idx], h["sizes"], **kw)
            if h["none"]:
                assert got == (None, None, None, None), f"tuple {k}"
                continue
            for name, g in zip(("min_d", "max_d", "min_point", "max_point"), got):
                w = want[f"hand{k}_{name}"]
                assert g.dtype == np.float64 and g.shape == w.shape
                if name.endswith("point"):
                    assert np.array_equal(g, w), f"tuple {k} {name}"
            M = MR.visible_depths(*md_tiny()[4], idx, h["K"], R, t, h["sizes"])
            err = max((np.abs(got[0] - want[f"hand{k}_min_d"]) / M["M_min"]).max(), (np.abs(got[1] - want[f"hand{k}_max_d"]) / M["M_max"]).max())
            print(f"tuple {k}: worst depth error against the reference {err:.3e} M")
            assert err <= BAR
    with pytest.raises(KeyError):
        CU.compute_min_max_depth_visible(points, [keys[0], keys[1], 99999], want["hand0_K"], R[:3], t[:3], want["hand0_sizes"], images=images)


def test_mine_tuples_returns_the_references_tuples(env):
    from wild_deep_mvs_amd.preprocess import mine_tuples
    cameras, images, points, want, flat, (K, R, t, _) = md_tiny()
    np.random.seed(int(want["seed"]))
    got = mine_tuples(cameras, images, points, nb_src=int(want["nb_src"]), nb_per_scene=int(want["nb_per_scene"]),
                      nb_points_thresh=int(want["nb_points_thresh"]), triangulation_angle_threshold=float(want["triangulation_angle_threshold"]),
                      usable=want["usable"], has_depth=want["has_depth"], image_sizes=want["image_sizes"], min_size=int(want["min_size"]))
    assert np.random.random() == float(want["rng_after"]), "the generator is left where the script leaves it"
    assert [m["idx_list"] for m in got] == want["mined_idx"].tolist()
    assert [[m["ref"]] + m["srcs"] for m in got] == want["mined_ids"].tolist()
    for k, m in enumerate(got):
        assert m["K"].dtype == np.float32 and np.array_equal(m["K"], want["mined_K"][k])
        assert np.array_equal(m["sizes"], want["mined_sizes"][k])
        assert np.array_equal(m["R"], R[m["idx_list"]]) and np.array_equal(m["t"], t[m["idx_list"]]) and m["t"].shape == (len(m["idx_list"]), 3, 1)
        M = MR.visible_depths(*flat, m["idx_list"], m["K"], R, t, m["sizes"])
        err = max((np.abs(m["min_d"] - want["mined_min_d"][k]) / M["M_min"]).max(), (np.abs(m["max_d"] - want["mined_max_d"][k]) / M["M_max"]).max())
        print(f"mined tuple {k}: worst depth error against the reference {err:.3e} M")
        assert err <= BAR
    # a smaller chunk of reference images per launch changes nothing, the generator's state included
    import wild_deep_mvs_amd.preprocess as PP
    chunk = PP.REF_CHUNK
    try:
        PP.REF_CHUNK = 2
        rng = np.random.RandomState(int(want["seed"]))
        again = mine_tuples(cameras, images, points, nb_src=int(want["nb_src"]), nb_per_scene=int(want["nb_per_scene"]),
                            nb_points_thresh=int(want["nb_points_thresh"]), usable=want["usable"], has_depth=want["has_depth"],
                            image_sizes=want["image_sizes"], rng=rng)
    finally:
        PP.REF_CHUNK = chunk
    assert [m["idx_list"] for m in again] == want["mined_idx"].tolist() and rng.random_sample() == float(want["rng_after"])
    assert all(np.array_equal(a["min_d"], b["min_d"]) and np.array_equal(a["max_d"], b["max_d"]) for a, b in zip(again, got))


def test_two_calls_give_identical_bits(env):
    _, ops, _ = env
    sc, (tuples, K, sizes) = MR.scene_70(7, 5)
    a, b = _run(ops, sc, tuples, K, sizes), _run(ops, sc, tuples, K, sizes)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_argument_errors(env):
    _, ops, _ = env
    sc, (tuples, K, sizes) = MR.scene_70(3, 10)
    xyz, off, img, R, t = _model(sc)
    ok = dict(tuples=_d(tuples, torch.int32), K=_d(K, torch.float32), sizes=_d(sizes, torch.float64))
    call = lambda **kw: ops.tuple_visible_depths(xyz, off, img, kw.get("tuples", ok["tuples"]), kw.get("K", ok["K"]), R, t,
                                                 kw.get("sizes", ok["sizes"]))
    name = "tuple_visible_depths"
    with pytest.raises(ValueError, match=name + r".*V=2 outside \[3,32\]"):
        call(tuples=ok["tuples"][:, :2].contiguous(), K=ok["K"][:, :2].contiguous(), sizes=ok["sizes"][:, :2].contiguous())
    wide = torch.arange(33, dtype=torch.int32).cuda()[None]
    with pytest.raises(ValueError, match=name + r".*V=33 outside \[3,32\]"):
        call(tuples=wide, K=torch.zeros(1, 33, 3, 3).cuda(), sizes=torch.zeros(1, 33, 2, dtype=torch.float64).cuda())
    twice = ok["tuples"].clone()
    twice[1, 4] = twice[1, 0]
    with pytest.raises(ValueError, match=name + ".*twice"):
        call(tuples=twice)
    for bad in (70, -1):
        far = ok["tuples"].clone()
        far[2, 9] = bad
        with pytest.raises(ValueError, match=name + r".*tuples holds an index outside \[0,70\)"):
            call(tuples=far)
    with pytest.raises(ValueError, match=name + ".*tuples int32"):
        call(tuples=ok["tuples"].long())
    with pytest.raises(ValueError, match=name + ".*K fp32"):
        call(K=ok["K"].double())
    with pytest.raises(ValueError, match=name + ".*K fp32"):
        call(K=ok["K"][:2].contiguous())
    with pytest.raises(ValueError, match=name + ".*sizes fp64"):
        call(sizes=ok["sizes"].float())
    with pytest.raises(ValueError, match=name + ".*xyz fp64"):
        ops.tuple_visible_depths(xyz.float(), off, img, ok["tuples"], ok["K"], R, t, ok["sizes"])
    with pytest.raises(ValueError, match=name + ".*track_off must have"):
        ops.tuple_visible_depths(xyz, off[:-1].contiguous(), img, ok["tuples"], ok["K"], R, t, ok["sizes"])
    torch.cuda.synchronize()                                   # no GPU error is left behind
    _check(_run(ops, sc, tuples, K, sizes), MR.visible_depths_batch(sc["xyz"], sc["track_off"], sc["track_img"], tuples, K, sc["R"], sc["t"], sizes),
           "after the errors")


def test_mine_tuples_raises_on_an_image_twice_in_a_track(env):
    from wild_deep_mvs_amd.preprocess import mine_tuples
    cameras, images, points = md_tiny()[:3]
    pid = next(iter(points))
    twice = dict(points)
    twice[pid] = points[pid]._replace(image_ids=np.concatenate([points[pid].image_ids, points[pid].image_ids[:1]]))
    with pytest.raises(ValueError, match="holds an image more than once"):
        mine_tuples(cameras, images, twice, nb_src=4, nb_per_scene=2)
    torch.cuda.synchronize()
