"""Depth-map fusion without a GPU: the PLY writer against the reference's own output, and the fusion rule (tests/_fusion_ref.py, the
yardstick of csrc/depth_fusion.hip) on an exact plane scene, where what it must emit follows from the geometry."""
import os

import numpy as np
import pytest

from tests import _fusion_ref as FR
from tests._util import GOLDEN


def _golden_arrays():
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_golden_fusion", os.path.join(GOLDEN, "gen_golden_fusion.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.golden_arrays()


def test_ply_writer_matches_the_reference_bytes(tmp_path):
    from wild_deep_mvs_amd.utils.point_cloud import write_point_cloud
    xyz, rgb = _golden_arrays()
    path = tmp_path / "points.ply"
    write_point_cloud(path, xyz, rgb)
    want = open(os.path.join(GOLDEN, "fusion_points.ply"), "rb").read()
    assert path.read_bytes() == want
    data = FR.read_ply(path)
    assert data.dtype.names == ("x", "y", "z", "red", "green", "blue")
    np.testing.assert_array_equal(np.stack([data[c] for c in "xyz"], axis=1), xyz)
    np.testing.assert_array_equal(np.stack([data[c] for c in ("red", "green", "blue")], axis=1), rgb)


def test_ply_writer_empty_cloud_and_bad_colours(tmp_path):
    from wild_deep_mvs_amd.utils.point_cloud import write_point_cloud
    write_point_cloud(tmp_path / "e.ply", np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint8))
    assert len(FR.read_ply(tmp_path / "e.ply")) == 0
    with pytest.raises(ValueError):
        write_point_cloud(tmp_path / "b.ply", np.zeros((2, 3), np.float32), np.zeros((2, 3), np.int32))


def _exact_scene(V=5, H=36, W=48):
    from wild_deep_mvs_amd import ops, synthetic
    sc = synthetic.make_fusion_scene(V, H, W, seed=0, exact=True, spacing=0.3)
    cams = ops.geo_filter_cams(sc["K"], sc["R"], sc["t"]).numpy()
    return sc, [d.numpy() for d in sc["depths"]], [c.numpy() for c in sc["colors"]], cams


def _rounding_bound(sc, cams, i):
    """Largest disparity change that rounding a projection to the nearest pixel can cause in view i's pass: on a plane, 1/depth is
    affine in the pixel coordinates of each view (1/d = n.(R^T K^-1 p) / (c0 - n.c)), so half a pixel in x and in y moves it by at
    most (|d(1/d)/dx| + |d(1/d)/dy|) / 2; times f_i |c_i - c_j|."""
    K, Ki, R, t = FR.cam_parts(cams)
    centre = -np.einsum("nji,nj->ni", R, t)
    n, c0 = sc["n"], sc["c0"]
    worst = 0.0
    for j in range(len(K)):
        if j == i:
            continue
        g = (n @ R[j].T @ Ki[j]) / (c0 - n @ centre[j])          # 1/d = g . (x, y, 1)
        fb = K[i, 0, 0] * np.linalg.norm(centre[i] - centre[j])
        worst = max(worst, fb * 0.5 * (abs(g[0]) + abs(g[1])))
    return worst


def test_rule_on_an_exact_plane():
    sc, depths, colors, cams = _exact_scene()
    V = len(depths)
    thr = 1.5 * max(_rounding_bound(sc, cams, i) for i in range(V)) + 1e-6
    nc = 2
    used = [np.zeros(d.shape, np.uint8) for d in depths]
    r0 = FR.fuse_pass(0, depths, colors, cams, used, disp_thresh=thr, num_consistent=nc)
    # pass 0: exactly the pixels that land (z > 0, inside, valid depth) in at least nc other views
    K, Ki, R, t = FR.cam_parts(cams)
    h, w = depths[0].shape
    ys, xs = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    X = FR.unproject(Ki[0], R[0], t[0], xs, ys, depths[0].astype(np.float64))
    seen = np.zeros((h, w), np.int64)
    for j in range(1, V):
        P = (X @ R[j].T + t[j]) @ K[j].T
        u, v = np.floor(P[..., 0] / P[..., 2] + 0.5), np.floor(P[..., 1] / P[..., 2] + 0.5)
        hj, wj = depths[j].shape
        seen += (P[..., 2] > 0) & (u >= 0) & (u < wj) & (v >= 0) & (v < hj)
    np.testing.assert_array_equal(r0["n"], seen)
    np.testing.assert_array_equal(r0["emit"], seen >= nc)
    assert 0.3 < r0["emit"].mean() < 1.0
    # every emitted point is on the plane; colours are the texture's (the views agree on it up to the rounded position)
    xyz, rgb, view, pix, passes = FR.fuse_all(depths, colors, cams, disp_thresh=thr, num_consistent=nc)
    assert len(xyz) > r0["emit"].sum()
    resid = np.abs(xyz @ sc["n"] - sc["c0"]) / sc["c0"]
    assert resid.max() < 1e-5, resid.max()
    assert rgb.min() >= 0 and rgb.max() <= 255
    # later passes emit only what the earlier passes did not consume
    used = [np.zeros(d.shape, np.uint8) for d in depths]
    for i in range(V):
        r = FR.fuse_pass(i, depths, colors, cams, used, disp_thresh=thr, num_consistent=nc)
        assert not (r["emit"] & (used[i] != 0)).any()
        if i > 0:
            assert r["emit"].sum() < r0["emit"].sum()
        for j in range(V):           # a pass marks only other views, and only adds marks
            assert (r["used"][j] >= used[j]).all()
            if j == i:
                np.testing.assert_array_equal(r["used"][j], used[j])
        used = r["used"]
    # more consistent views than there are other views: nothing
    xyz_none = FR.fuse_all(depths, colors, cams, disp_thresh=thr, num_consistent=V)[0]
    assert len(xyz_none) == 0


def test_rule_threshold_below_the_rounding_bound_loses_points():
    """The bound above is what makes the exact-plane check meaningful: far below it, rounding alone breaks consistency."""
    sc, depths, colors, cams = _exact_scene()
    bound = max(_rounding_bound(sc, cams, i) for i in range(len(depths)))
    used = [np.zeros(d.shape, np.uint8) for d in depths]
    hi = FR.fuse_pass(0, depths, colors, cams, used, disp_thresh=1.5 * bound + 1e-6, num_consistent=2)["emit"].sum()
    lo = FR.fuse_pass(0, depths, colors, cams, used, disp_thresh=0.05 * bound, num_consistent=2)["emit"].sum()
    assert lo < hi


def test_fusion_entry_points_exist_and_check_inputs():
    """The ABI constant and the ops entry points; input checks that need no device."""
    import torch
    from wild_deep_mvs_amd import _lib as L, ops
    from wild_deep_mvs_amd.evaluation import fusibile  # noqa: F401
    assert L.FUSE_MAX_VIEWS == 64 and "pscv_fuse_depth_pass" in L.EXPORTS
    with pytest.raises(ValueError):
        ops.pack_rgba8(torch.zeros(4, 4, 3, dtype=torch.int32))
    packed = ops.pack_rgba8(torch.tensor([[[1, 2, 3]]], dtype=torch.uint8))
    assert packed.dtype == torch.int32 and int(packed[0, 0]) == 1 | (2 << 8) | (3 << 16)
    with pytest.raises((ValueError, RuntimeError)):
        ops.fuse_depth_maps([torch.zeros(4, 4)], [torch.zeros(4, 4, 3, dtype=torch.uint8)], torch.zeros(1, 30))
