"""CPU: the numpy rule of the COLMAP-style fusion with normal maps (tests/_colmap_fusion_normals_ref.py, INTEGRATION.md section
2g "with normal maps") on hand-built cases, its agreement with the normal-free rule when the test is off, its deviation from
COLMAP's sequential loop on ``make_normal_fusion_scene`` (the bound 2g states), and the host logic of
``evaluation.colmap_fusion`` under ``args.colmap`` that runs before anything reaches the device."""
import math
from argparse import Namespace

import numpy as np
import pytest
import torch

from tests import _colmap_fusion_normals_ref as NR
from tests import _colmap_fusion_ref as CR

KW = dict(max_depth_error=0.01, max_reproj_error=0.9)     # (co-located views: the window neighbours lie at exactly 1 pixel)


def _rig(n, h, w, angles_deg, *, depth=5.0):
    """n co-located cameras (R = I, so camera frame = world frame) looking along +z at the plane z = depth; view v has the
    constant normal (0, -sin a_v, -cos a_v): a_v degrees away from (0, 0, -1), all in one plane."""
    from wild_deep_mvs_amd import ops
    K = torch.tensor([[[20.0, 0.0, w / 2.0], [0.0, 20.0, h / 2.0 + 0.13], [0.0, 0.0, 1.0]]] * n, dtype=torch.float32)
    cams = ops.geo_filter_cams(K, torch.eye(3).repeat(n, 1, 1), torch.zeros(n, 3, 1)).numpy()
    depths = [np.full((h, w), depth, np.float32) for _ in range(n)]
    colors = [np.full((h, w, 3), 10 * v, np.uint8) for v in range(n)]
    normals = [np.broadcast_to(_nrm(a), (h, w, 3)).copy() for a in angles_deg]
    return depths, colors, normals, cams


def _nrm(a):
    return np.array([0.0, -math.sin(math.radians(a)), -math.cos(math.radians(a))], np.float32) if a is not None else np.zeros(3, np.float32)


def _fresh(depths):
    return [np.zeros(d.shape, np.uint8) for d in depths]


def test_world_normal_and_min_cos():
    from wild_deep_mvs_amd import ops
    a = 0.3
    R = torch.tensor([[[math.cos(a), 0.0, math.sin(a)], [0.0, 1.0, 0.0], [-math.sin(a), 0.0, math.cos(a)]]], dtype=torch.float32)
    cams = ops.geo_filter_cams(torch.eye(3)[None], R, torch.zeros(1, 3, 1)).numpy()
    from tests._fusion_ref import cam_rows
    n = np.array([0.1, -0.2, -0.9], np.float32)
    w = NR.world_normals(cam_rows(cams)[0], n)
    assert w.dtype == np.float32
    np.testing.assert_allclose(w, R[0].numpy().astype(np.float64).T @ n.astype(np.float64), rtol=0, atol=1e-7)
    assert NR.min_cos_of(180.0) == -1.0 and abs(NR.min_cos_of(10.0) - math.cos(math.radians(10.0))) < 1e-15


def test_a_pixel_15_degrees_off_joins_at_20_and_not_at_10():
    depths, colors, normals, cams = _rig(2, 4, 6, [0.0, 15.0])
    ov = [[1], [0]]
    r = NR.parallel_pass(0, depths, colors, normals, cams, ov, [False] * 2, _fresh(depths), min_num_pixels=2, max_normal_error=10.0, **KW)
    assert len(r["xyz"]) == 0 and r["fused"][0].all() and not r["fused"][1].any()
    assert r["tested"] == 24 and r["rejected"] == 24            # depth and reprojection passed: the normal test alone refused
    r = NR.parallel_pass(0, depths, colors, normals, cams, ov, [False] * 2, _fresh(depths), min_num_pixels=2, max_normal_error=20.0, **KW)
    assert len(r["xyz"]) == 24 and r["fused"][1].all() and r["rejected"] == 0
    assert r["margin"] >= 1e-9
    # the literal sequential loop agrees on both
    for err, want in ((10.0, 0), (20.0, 24)):
        sx, _, _, _ = NR.sequential_fuse(depths, colors, normals, cams, ov, min_num_pixels=2, max_normal_error=err, **KW)
        assert len(sx) == want


def test_a_refused_pixel_stays_unfused_and_seeds_its_own_cluster():
    depths, colors, normals, cams = _rig(2, 4, 6, [0.0, 15.0])
    xyz, nor, rgb, view, margin, passes = NR.parallel_fuse(depths, colors, normals, cams, [[1], [0]], min_num_pixels=1,
                                                           max_normal_error=10.0, **KW)
    assert view.tolist() == [0] * 24 + [1] * 24
    assert not passes[0][1]["fused"][1].any() and passes[1][1]["fused"][1].all()
    np.testing.assert_allclose(nor[:24], np.broadcast_to(_nrm(0.0), (24, 3)), atol=1e-7)
    np.testing.assert_allclose(nor[24:], np.broadcast_to(_nrm(15.0), (24, 3)), atol=1e-7)
    sx, sn, _, sv = NR.sequential_fuse(depths, colors, normals, cams, [[1], [0]], min_num_pixels=1, max_normal_error=10.0, **KW)
    assert sv.tolist() == view.tolist()


def test_the_normal_test_is_against_the_seed_not_the_parent():
    """A chain 0 -> 8 -> 16 degrees: view 2 is entered from view 1 (8 degrees from it) but lies 16 degrees from the seed."""
    depths, colors, normals, cams = _rig(3, 4, 6, [0.0, 8.0, 16.0])
    ov = [[1], [2], []]
    r = NR.parallel_pass(0, depths, colors, normals, cams, ov, [False] * 3, _fresh(depths), min_num_pixels=3, max_normal_error=10.0, **KW)
    assert len(r["xyz"]) == 0 and r["fused"][1].all() and not r["fused"][2].any()
    r = NR.parallel_pass(0, depths, colors, normals, cams, ov, [False] * 3, _fresh(depths), min_num_pixels=2, max_normal_error=10.0, **KW)
    assert len(r["xyz"]) == 24 and not r["fused"][2].any()
    sx, _, _, _ = NR.sequential_fuse(depths, colors, normals, cams, ov, min_num_pixels=3, max_normal_error=10.0, **KW)
    assert len(sx) == 0
    r = NR.parallel_pass(0, depths, colors, normals, cams, ov, [False] * 3, _fresh(depths), min_num_pixels=3, max_normal_error=17.0, **KW)
    assert len(r["xyz"]) == 24 and r["fused"][2].all()


def test_median_normal_of_an_odd_and_an_even_cluster():
    ov = [[1, 2], [0, 2], [0, 1]]
    depths, colors, normals, cams = _rig(3, 2, 3, [0.0, 8.0, 4.0])
    r = NR.parallel_pass(0, depths, colors, normals, cams, ov, [False] * 3, _fresh(depths), min_num_pixels=3, max_normal_error=10.0, **KW)
    mid = _nrm(4.0).astype(np.float64)                       # per component the middle of 0, 4 and 8 degrees
    want = (mid / np.sqrt(mid[0] * mid[0] + mid[1] * mid[1] + mid[2] * mid[2])).astype(np.float32)
    assert len(r["normal"]) == 6
    np.testing.assert_array_equal(r["normal"], np.broadcast_to(want, (6, 3)))
    depths, colors, normals, cams = _rig(2, 2, 3, [0.0, 8.0])
    r = NR.parallel_pass(0, depths, colors, normals, cams, [[1], [0]], [False] * 2, _fresh(depths), min_num_pixels=2,
                         max_normal_error=10.0, **KW)
    a, b = _nrm(0.0), _nrm(8.0)
    g = ((a + b) * np.float32(0.5)).astype(np.float64)
    want = (g / np.sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2])).astype(np.float32)
    assert len(r["normal"]) == 6
    np.testing.assert_array_equal(r["normal"], np.broadcast_to(want, (6, 3)))
    assert abs(float(np.linalg.norm(r["normal"][0].astype(np.float64))) - 1.0) < 1e-6


def test_a_zero_normal_seed_emits_nothing():
    depths, colors, normals, cams = _rig(2, 4, 6, [None, 0.0])
    for mnp in (1, 2):
        r = NR.parallel_pass(0, depths, colors, normals, cams, [[1], [0]], [False] * 2, _fresh(depths), min_num_pixels=mnp,
                             max_normal_error=10.0, **KW)
        assert len(r["xyz"]) == 0 and r["fused"][0].all() and not r["fused"][1].any()
    sx, _, _, _ = NR.sequential_fuse(depths, colors, normals, cams, [[1], [0]], min_num_pixels=1, max_normal_error=10.0, **KW)
    assert len(sx) == 24            # view 1's pixels, seeding in their own pass; the 24 zero-normal seeds of view 0 are dropped
    normals[0][...] = np.nan        # a NaN fails the comparison, at any angle
    r = NR.parallel_pass(0, depths, colors, normals, cams, [[1], [0]], [False] * 2, _fresh(depths), min_num_pixels=1,
                         max_normal_error=180.0, **KW)
    assert len(r["xyz"]) == 0 and not r["fused"][1].any()


def test_test_off_and_constant_normals_give_the_normal_free_rule():
    """max_normal_error = 180 and constant maps float32(1/sqrt(3)): the fused masks, xyz, rgb and seed pixels of every pass are
    those of _colmap_fusion_ref.parallel_pass; the normals agree to 1e-6 (its constant is a float64 literal)."""
    from wild_deep_mvs_amd import ops, synthetic
    sc = synthetic.make_yfcc_fusion_scene(5, 24, 32, seed=3)
    cams = ops.geo_filter_cams(sc["K"], sc["R"], sc["t"]).numpy()
    d, c = [x.numpy() for x in sc["depths"]], [x.numpy() for x in sc["colors"]]
    nm = [np.full(x.shape + (3,), np.float32(1.0 / np.sqrt(3.0)), np.float32) for x in d]
    kw = dict(max_depth_error=0.01, max_reproj_error=1.0, min_num_pixels=3)
    *_, margin, want = CR.parallel_fuse(d, c, cams, sc["overlap"], **kw)
    *_, margin_n, got = NR.parallel_fuse(d, c, nm, cams, sc["overlap"], max_normal_error=180.0, **kw)
    assert margin >= 1e-9 and margin_n >= 1e-9
    total = 0
    for (v, a), (u, b) in zip(want, got):
        assert v == u and b["rejected"] == 0
        for x, y in zip(a["fused"], b["fused"]):
            np.testing.assert_array_equal(x, y)
        np.testing.assert_array_equal(a["pixel"], b["pixel"])
        np.testing.assert_array_equal(a["xyz"].view(np.uint32), b["xyz"].view(np.uint32))
        np.testing.assert_array_equal(a["rgb"], b["rgb"])
        np.testing.assert_allclose(a["normal"], b["normal"], rtol=0, atol=1e-6)
        total += len(a["xyz"])
    assert total > 100


@pytest.mark.parametrize("V,H,W,r", [(5, 24, 32, 1.0), (5, 24, 32, 2.0), (10, 16, 24, 1.0)])
def test_parallel_rule_against_the_sequential_loop_with_normals(V, H, W, r):
    """The bound of INTEGRATION.md section 2g (tests/test_colmap_fusion_cpu.py), with the normal test on at 10 degrees on
    ``make_normal_fusion_scene``: 1.0-1.6 x the sequential loop's points, and a symmetric Chamfer distance below half the footprint
    of one pixel at the scene's depth (the median true depth over the mean focal length)."""
    from wild_deep_mvs_amd import ops, synthetic
    sc = synthetic.make_normal_fusion_scene(V, H, W, seed=11)
    cams = ops.geo_filter_cams(sc["K"], sc["R"], sc["t"]).numpy()
    d, c, nm = ([x.numpy() for x in sc[k]] for k in ("depths", "colors", "normals"))
    kw = dict(max_depth_error=0.01, max_reproj_error=r, min_num_pixels=3, max_normal_error=10.0)
    px, _, _, _, margin, passes = NR.parallel_fuse(d, c, nm, cams, sc["overlap"], **kw)
    sx, _, _, _ = NR.sequential_fuse(d, c, nm, cams, sc["overlap"], **kw)
    assert margin >= 1e-9
    assert sum(p["rejected"] for _, p in passes) > 0
    footprint = float(np.median(sc["depth_gt"].numpy())) / float(sc["K"][:, 0, 0].mean())
    ch = CR.chamfer(px, sx)
    print(f"V={V} {H}x{W} r={r}: parallel {len(px)}, sequential {len(sx)}, ratio {len(px) / len(sx):.3f}, Chamfer / footprint "
          f"{ch / footprint:.3f}")
    assert len(sx) <= len(px) <= 1.6 * len(sx), (len(px), len(sx))
    assert ch < 0.5 * footprint, (ch, footprint)


def test_normal_fusion_scene_has_what_it_promises():
    from wild_deep_mvs_amd import synthetic
    sc = synthetic.make_normal_fusion_scene(5, 24, 32, seed=3)
    again = synthetic.make_normal_fusion_scene(5, 24, 32, seed=3)
    R = sc["R"].numpy().astype(np.float64)
    for v in range(5):
        d, n = sc["depths"][v].numpy(), sc["normals"][v].numpy()
        assert d.dtype == np.float32 and n.dtype == np.float32 and n.shape == d.shape + (3,) and sc["colors"][v].dtype == torch.uint8
        assert torch.equal(sc["normals"][v], again["normals"][v]) and torch.equal(sc["depths"][v], again["depths"][v])
        gone = d == 0
        assert gone.sum() >= 15 and (n[gone] == 0).all()
        np.testing.assert_allclose(np.linalg.norm(n[~gone], axis=-1), 1.0, atol=1e-6)
        w = n.astype(np.float64) @ R[v]                                          # R^T n per pixel
        ang = np.degrees(np.arccos(np.clip((w * sc["normal_world"][v].numpy()).sum(-1), -1, 1)))
        rot = sc["rotated"][v].numpy()
        if v == 1:
            assert rot.sum() == 12 * 16 and (ang[rot & ~gone] > 15).all() and (ang[rot & ~gone] < 35).all()
            same = ~gone & rot                                                  # the turned block keeps its true depth
            np.testing.assert_array_equal(d[same], sc["depth_gt"][v].numpy()[same])
        else:
            assert not rot.any()
        # Gaussian tangent jitter of 2.5 degrees per axis: a Rayleigh angle, median 2.9 degrees, 99th percentile 7.6
        assert np.median(ang[~gone & ~rot]) < 5 and np.percentile(ang[~gone & ~rot], 99) < 10
    out = sc["depths"][0].numpy() / np.maximum(sc["depth_gt"][0].numpy(), 1e-9)
    assert (np.abs(out - 1.25) < 1e-6).sum() >= 10


# ---- evaluation.colmap_fusion under args.colmap: what happens before the device is touched ----------------------------------------
def _args(tmp_path, **kw):
    base = dict(model=None, nviews=3, data_path=str(tmp_path), scene="sceneB_3", downscale=1, colmap=True, filter=False,
                upsample=False, prob_threshold=0.5, fusion_depth_threshold=0.01, fusion_max_reproj_error=1.0, fusion_num_consistent=3,
                override=True, dataset="yfcc")
    base.update(kw)
    return Namespace(**base)


def _batches(V, h, w):
    K = torch.tensor([[20.0, 0.0, w / 2.0], [0.0, 20.0, h / 2.0], [0.0, 0.0, 1.0]])
    return [{"filename": [f"{v:08d}"], "imgs": torch.rand(1, 1, 3, h, w), "K": K[None, None], "R": torch.eye(3)[None, None],
             "t": torch.zeros(1, 1, 3, 1)} for v in range(V)]


def _write_maps(folder, normal_dir, V, h, w, *, normal_shape=None, skip_normal=()):
    from wild_deep_mvs_amd.utils.colmap_array import write_array
    folder.mkdir(parents=True, exist_ok=True)
    normal_dir.mkdir(parents=True, exist_ok=True)
    for v in range(V):
        d = np.full((h, w), 5.0, np.float32)
        np.savez(folder / f"{v:08d}_out.npz", depthmap=d, probability=np.ones_like(d))
        if v not in skip_normal:
            nh, nw = normal_shape or (h, w)
            write_array(np.broadcast_to(np.array([0.0, 0.0, -1.0], np.float32), (nh, nw, 3)).copy(),
                        normal_dir / f"{v:08d}.jpg.geometric.bin")


def test_without_normal_maps_the_colmap_branch_refuses_and_leaves_the_ply(tmp_path):
    from wild_deep_mvs_amd.evaluation import colmap_fusion as CF
    args = _args(tmp_path)
    ply = tmp_path / "Points" / "None_3" / "None_3sceneB_3.ply"
    ply.parent.mkdir(parents=True)
    ply.write_bytes(b"kept")
    with pytest.raises(NotImplementedError, match="depthmap_colmap"):
        CF.colmap_fusion(_batches(3, 4, 6), args)
    assert ply.read_bytes() == b"kept"
    assert not (tmp_path / "IntRes").exists()
    assert CF.MAX_NORMAL_ERROR == 10.0


def test_depth_folder_fallback_and_the_missing_normal_file(tmp_path, capsys):
    """No IntRes/depthmaps/None_3 folder: the maps of depthmap_colmap under direct_depthmaps/colmap are read, and the run says so.
    View 1 has a depth map and no normal map: FileNotFoundError (before anything reaches the device)."""
    from wild_deep_mvs_amd.evaluation import colmap_fusion as CF
    args = _args(tmp_path)
    normal_dir = tmp_path / "IntRes" / "colmap_dense" / "sceneB_3" / "stereo" / "normal_maps"
    direct = tmp_path / "IntRes" / "direct_depthmaps" / "colmap" / "sceneB_3"
    _write_maps(direct, normal_dir, 3, 4, 6, skip_normal=(1,))
    with pytest.raises(FileNotFoundError, match="00000001"):
        CF.colmap_fusion(_batches(3, 4, 6), args)
    out = capsys.readouterr().out
    assert str(direct) in out and "Could not open" not in out
    # the reference's folder wins when it exists (here: empty, so every view is skipped with the reference's message)
    ref = tmp_path / "IntRes" / "depthmaps" / "None_3" / "sceneB_3"
    ref.mkdir(parents=True)
    with pytest.raises(Exception):
        CF.colmap_fusion(_batches(3, 4, 6), args)
    out = capsys.readouterr().out
    assert str(ref) in out and str(direct) not in out and out.count("Could not open") == 3


def test_a_normal_map_of_another_size_is_refused(tmp_path):
    from wild_deep_mvs_amd.evaluation import colmap_fusion as CF
    args = _args(tmp_path)
    normal_dir = tmp_path / "IntRes" / "colmap_dense" / "sceneB_3" / "stereo" / "normal_maps"
    _write_maps(tmp_path / "IntRes" / "direct_depthmaps" / "colmap" / "sceneB_3", normal_dir, 3, 4, 6, normal_shape=(8, 12))
    with pytest.raises(ValueError, match=r"\(8, 12, 3\).*\(4, 6\)"):
        CF.colmap_fusion(_batches(3, 4, 6), args)
    # the same maps under args.upsample x 2 match the upsampled depth: the shape check passes and the fusion itself is reached
    args = _args(tmp_path, upsample=True, downscale=2)
    seen = {}

    def fake(depths, colors, cams, overlap, **kw):
        seen.update(kw)
        raise RuntimeError("reached the device call")

    from wild_deep_mvs_amd import ops
    mp = pytest.MonkeyPatch()
    mp.setattr(ops, "colmap_fuse", fake)
    mp.setattr(torch.Tensor, "cuda", lambda self, *a, **k: self)
    mp.setattr(ops, "geo_filter_cams", lambda K, R, t: torch.zeros(len(K), 30))
    try:
        with pytest.raises(RuntimeError, match="reached the device call"):
            CF.colmap_fusion(_batches(3, 8, 12), args)
    finally:
        mp.undo()
    assert seen["max_normal_error"] == 10.0 and len(seen["normals"]) == 3 and tuple(seen["normals"][0].shape) == (8, 12, 3)


def test_ops_signature_accepts_normals():
    import inspect
    from wild_deep_mvs_amd import ops
    for fn in (ops.colmap_fuse, ops.colmap_fuse_pass):
        p = inspect.signature(fn).parameters
        assert p["normals"].default is None and p["max_normal_error"].default is None
    p = inspect.signature(ops._ColmapRun.__init__).parameters
    assert list(p)[1:8] == ["depths", "colors", "cams", "overlap", "fused", "capacity", "params"]
    assert p["normals"].kind is inspect.Parameter.KEYWORD_ONLY and p["max_normal_error"].kind is inspect.Parameter.KEYWORD_ONLY
