"""CPU: the numpy rule of the COLMAP-style fusion (tests/_colmap_fusion_ref.py) on hand-built cases,
its deviation from COLMAP's sequential loop on small scenes (the bound 2g states), the COLMAP model reader against a model
written by the reference's own writer (tests/golden/colmap_tiny, gen_golden_colmap.py), the overlap order and the PLY layout."""
import os

import numpy as np
import pytest
import torch

from tests import _colmap_fusion_ref as CR

HERE = os.path.dirname(os.path.abspath(__file__))
KW = dict(max_depth_error=0.01, max_reproj_error=1.0)


def _rig(n, h, w, *, f=20.0, cx=None, depth=5.0):
    """n cameras at the origin looking along +z at the plane z = depth; view v has focal f_v and principal point cx_v."""
    from wild_deep_mvs_amd import ops
    fs = [f] * n if np.isscalar(f) else list(f)
    cxs = [w / 2.0] * n if cx is None else list(cx)
    K = torch.tensor([[[fs[v], 0.0, cxs[v]], [0.0, fs[v], h / 2.0 + 0.13], [0.0, 0.0, 1.0]] for v in range(n)], dtype=torch.float32)
    R = torch.eye(3).repeat(n, 1, 1)
    t = torch.zeros(n, 3, 1)
    cams = ops.geo_filter_cams(K, R, t).numpy()
    depths = [np.full((h, w), depth, np.float32) for _ in range(n)]
    colors = [np.full((h, w, 3), 10 * v, np.uint8) for v in range(n)]
    return depths, colors, cams


def _fresh(depths):
    return [np.zeros(d.shape, np.uint8) for d in depths]


def test_find_next_image_order():
    assert CR.find_next_image_order([[2, 1], [0], [3], []]) == [0, 2, 3, 1]
    assert CR.find_next_image_order([[], [], []]) == [0, 1, 2]
    assert CR.find_next_image_order([[1], [0], [1, 0]]) == [0, 1, 2]
    from wild_deep_mvs_amd import ops
    assert ops.find_next_image_order([[2, 1], [0], [3], []]) == [0, 2, 3, 1]
    assert ops.colmap_overlap_lists(np.array([[1, 1, 0], [0, 0, 1], [1, 0, 0]], bool), 3) == [[1], [2], [0]]


def test_medians_even_and_odd():
    assert CR.median_f32([3.0, 1.0, 2.0]) == np.float32(2.0)
    assert CR.median_f32([4.0, 1.0, 2.0, 3.0]) == np.float32(2.5)
    a, b = np.float32(1.0000001), np.float32(1.0000002)
    assert CR.median_f32([a, b]) == np.float32((a + b) * np.float32(0.5))
    assert CR.median_u8([10, 11]) == 11 and CR.median_u8([10, 12]) == 11 and CR.median_u8([9, 1, 200]) == 9


def test_reachable_only_at_depth_two_and_the_depth_cap():
    """Three co-located views: view 2 is not in overlap[0] but follows view 1, so a seed of view 0 reaches it at depth 2; with
    max_traversal_depth 2 it does not."""
    depths, colors, cams = _rig(3, 4, 6)
    ov = [[1], [2], []]
    r = CR.parallel_pass(0, depths, colors, cams, ov, [False] * 3, _fresh(depths), min_num_pixels=3, **KW)
    assert len(r["xyz"]) == 24 and r["fused"][2].all()
    r = CR.parallel_pass(0, depths, colors, cams, ov, [False] * 3, _fresh(depths), min_num_pixels=3, max_traversal_depth=2, **KW)
    assert len(r["xyz"]) == 0 and r["fused"][1].all() and not r["fused"][2].any()
    r = CR.parallel_pass(0, depths, colors, cams, ov, [False] * 3, _fresh(depths), min_num_pixels=1, max_traversal_depth=1, **KW)
    assert len(r["xyz"]) == 24 and not r["fused"][1].any()


def test_contested_pixel_goes_to_the_lower_seed_and_dropped_clusters_stay_marked():
    """View 1 has half the focal length: seeds x = 2k+1 and 2k+2 of view 0 both land on pixel k+1 of view 1; the lower seed
    takes it, the other's cluster is the seed alone -- dropped, but its seed pixel is fused."""
    depths, colors, cams = _rig(2, 1, 9, f=[20.0, 10.0], cx=[0.0, 0.1])
    depths[1] = depths[1][:, :5].copy()
    colors[1] = colors[1][:, :5].copy()
    r = CR.parallel_pass(0, depths, colors, cams, [[1], [0]], [False] * 2, _fresh(depths), min_num_pixels=2, **KW)
    assert r["pixel"].tolist() == [0, 1, 3, 5, 7]
    assert r["fused"][0].all() and r["fused"][1].all()
    assert r["margin"] >= 1e-9


def test_no_entry_into_processed_views():
    depths, colors, cams = _rig(3, 4, 6)
    ov = [[1, 2], [0, 2], [0, 1]]
    r = CR.parallel_pass(0, depths, colors, cams, ov, [False, True, False], _fresh(depths), min_num_pixels=2, **KW)
    assert not r["fused"][1].any() and r["fused"][2].all() and len(r["xyz"]) == 24
    # already-fused pixels neither seed nor join
    fz = _fresh(depths)
    fz[0][0] = 1
    fz[2][1] = 1
    r = CR.parallel_pass(0, depths, colors, cams, ov, [False] * 3, fz, min_num_pixels=3, **KW)
    assert len(r["xyz"]) == 12 and r["fused"][1][1:].all() and not r["fused"][1][0].any()


@pytest.mark.parametrize("V,H,W,r", [(5, 24, 32, 1.0), (5, 24, 32, 2.0), (10, 16, 24, 1.0)])
def test_parallel_rule_against_the_sequential_loop(V, H, W, r):
    """The bound INTEGRATION.md section 2g states: the parallel rule emits 1.0-1.6 x the sequential loop's points (its seeds
    never absorb neighbours of their own view, and seeds that lose a contest still emit smaller clusters), and the symmetric
    Chamfer distance between the clouds stays below half the footprint of one pixel at the scene's depth."""
    from wild_deep_mvs_amd import ops, synthetic
    sc = synthetic.make_yfcc_fusion_scene(V, H, W, seed=11)
    cams = ops.geo_filter_cams(sc["K"], sc["R"], sc["t"]).numpy()
    d, c = [x.numpy() for x in sc["depths"]], [x.numpy() for x in sc["colors"]]
    kw = dict(max_depth_error=0.01, max_reproj_error=r, min_num_pixels=3)
    px, _, _, _, margin, _ = CR.parallel_fuse(d, c, cams, sc["overlap"], **kw)
    sx, _, _, _ = CR.sequential_fuse(d, c, cams, sc["overlap"], **kw)
    assert margin >= 1e-9
    footprint = 4.0 / float(sc["K"][:, 0, 0].mean())
    assert len(sx) <= len(px) <= 1.6 * len(sx), (len(px), len(sx))
    assert CR.chamfer(px, sx) < 0.5 * footprint, (CR.chamfer(px, sx), footprint)


def test_colmap_model_reader_against_the_reference_writer():
    from wild_deep_mvs_amd.utils import colmap_model as CM
    gold = os.path.join(HERE, "golden", "colmap_tiny")
    images = CM.read_images_binary(os.path.join(gold, "images.bin"))
    points = CM.read_points3D_binary(os.path.join(gold, "points3D.bin"))
    assert {k: v.name for k, v in images.items()} == {3: "00000000.jpg", 1: "00000001.jpg", 7: "00000002.jpg", 2: "00000003.jpg"}
    assert images[3].point3D_ids.tolist() == [10, 11, 13, 15, -1]
    assert {k: v.image_ids.tolist() for k, v in points.items()} == {10: [3, 1], 11: [3, 1, 7], 12: [1, 7], 13: [3, 1, 7, 2],
                                                                    14: [7, 2], 15: [3, 7]}
    assert points[13].point2D_idxs.tolist() == [2, 3, 2, 0]
    names = ["00000000.jpg", "00000001.jpg", "00000002.jpg", "00000003.jpg"]
    counts = CM.shared_point_counts(gold, names)
    np.testing.assert_array_equal(counts, [[0, 3, 3, 1], [3, 0, 3, 1], [3, 3, 0, 2], [1, 1, 2, 0]])
    assert CM.overlap_from_counts(counts) == [[1, 2, 3], [0, 2, 3], [0, 1, 3], [2, 0, 1]]
    assert CM.overlap_from_counts(counts, 2) == [[1, 2], [0, 2], [0, 1], [2, 0]]


def test_colmap_ply_round_trip(tmp_path):
    from wild_deep_mvs_amd.utils.point_cloud import read_ply, write_colmap_point_cloud
    rng = np.random.default_rng(0)
    xyz = rng.standard_normal((17, 3)).astype(np.float32)
    nor = rng.standard_normal((17, 3)).astype(np.float32)
    rgb = rng.integers(0, 256, (17, 3), dtype=np.uint8)
    path = tmp_path / "fused.ply"
    write_colmap_point_cloud(path, xyz, nor, rgb)
    raw = path.read_bytes()
    assert raw.startswith(b"ply\nformat binary_little_endian 1.0\nelement vertex 17\nproperty float x\n")
    assert b"property float nz\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n" in raw
    data = read_ply(path)
    assert data.dtype.names == ("x", "y", "z", "nx", "ny", "nz", "red", "green", "blue")
    np.testing.assert_array_equal(np.stack([data[k] for k in "xyz"], 1), xyz)
    np.testing.assert_array_equal(np.stack([data[k] for k in ("nx", "ny", "nz")], 1), nor)
    np.testing.assert_array_equal(np.stack([data[k] for k in ("red", "green", "blue")], 1), rgb)
    from wild_deep_mvs_amd.evaluation.metrics import format_point_cloud
    assert format_point_cloud(data).shape == (17, 3)
