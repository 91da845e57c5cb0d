"""GPU: COLMAP-style stereo fusion (pscv_colmap_fuse_pass, csrc/colmap_fusion.hip) against the numpy rule of
tests/_colmap_fusion_ref.py, bit for bit: after every pass the fused masks and the point count match exactly and xyz, normal,
rgb and the seed pixels are equal.  Also determinism, the evaluation/colmap_fusion.py mirror feeding metrics.run, the capacity
check and every limit.  Scene decisions stay at least 1e-9 (relative) away from their thresholds, which each case asserts."""
from argparse import Namespace

import numpy as np
import pytest
import torch

from tests import _colmap_fusion_ref as CR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from wild_deep_mvs_amd import _lib as L, ops, synthetic
    L.lib()
    return L, ops, synthetic


def _inputs(ops, sc):
    cams = ops.geo_filter_cams(sc["K"], sc["R"], sc["t"])
    return [d.cuda() for d in sc["depths"]], [c.cuda() for c in sc["colors"]], cams.cuda(), cams.numpy()


CASES = {  # name: (V, H, W, scene options, fusion options)
    "n2": (2, 24, 32, {}, {"max_reproj_error": 1.0, "min_num_pixels": 2}),
    "n5_r1": (5, 24, 32, {}, {"max_reproj_error": 1.0, "min_num_pixels": 3}),
    "n5_r2": (5, 24, 32, {}, {"max_reproj_error": 2.0, "min_num_pixels": 3}),
    "n10_knn_r15": (10, 20, 28, {"overlap": "knn", "k_overlap": 3}, {"max_reproj_error": 1.5, "min_num_pixels": 3}),
    "n10_chain_td2": (10, 20, 28, {"overlap": "chain"}, {"max_reproj_error": 1.0, "min_num_pixels": 2, "max_traversal_depth": 2}),
    "n20": (20, 16, 20, {}, {"max_reproj_error": 1.0, "min_num_pixels": 3}),
    "n64": (64, 8, 10, {"spacing": 0.1}, {"max_reproj_error": 1.0, "min_num_pixels": 5}),
}


@pytest.mark.parametrize("case", list(CASES))
def test_each_pass_matches_the_rule(env, case):
    L, ops, synthetic = env
    V, H, W, sopt, fopt = CASES[case]
    sc = synthetic.make_yfcc_fusion_scene(V, H, W, seed=3, **sopt)
    depths, colors, cams, cams_np = _inputs(ops, sc)
    kw = dict(max_depth_error=0.01, **fopt)
    d_np, c_np = [d.numpy() for d in sc["depths"]], [c.numpy() for c in sc["colors"]]
    fused = [torch.zeros(d.shape, dtype=torch.uint8, device="cuda") for d in depths]
    processed, total, outs = [], 0, []
    order = ops.find_next_image_order(ops.colmap_overlap_lists(sc["overlap"], V))
    assert order == CR.find_next_image_order(sc["overlap"])
    for v in order:
        before = [f.cpu().numpy() for f in fused]
        want = CR.parallel_pass(v, d_np, c_np, cams_np, sc["overlap"], [u in processed for u in range(V)], before, **kw)
        assert want["margin"] >= 1e-9, f"pass {v}: a decision lies {want['margin']:.2e} from its threshold"
        xyz, nor, rgb, pix = ops.colmap_fuse_pass(v, depths, colors, cams, sc["overlap"], fused, processed=processed, **kw)
        torch.cuda.synchronize()
        for u in range(V):
            np.testing.assert_array_equal(fused[u].cpu().numpy(), want["fused"][u], err_msg=f"pass {v}: fused mask of view {u}")
        assert xyz.shape[0] == len(want["xyz"]), f"pass {v}"
        np.testing.assert_array_equal(pix.cpu().numpy(), want["pixel"])
        np.testing.assert_array_equal(xyz.cpu().numpy().view(np.uint32), want["xyz"].view(np.uint32))
        np.testing.assert_array_equal(nor.cpu().numpy().view(np.uint32), want["normal"].view(np.uint32))
        np.testing.assert_array_equal(rgb.cpu().numpy(), want["rgb"])
        total += xyz.shape[0]
        outs.append(xyz.cpu())
        processed.append(v)
    assert total > 20
    # the whole run is the passes in order
    xyz, nor, rgb, view = ops.colmap_fuse(depths, colors, cams, sc["overlap"], **kw)
    assert torch.equal(xyz.cpu(), torch.cat(outs))


def test_fusion_is_deterministic(env):
    L, ops, synthetic = env
    sc = synthetic.make_yfcc_fusion_scene(20, 48, 64, seed=7)
    depths, colors, cams, _ = _inputs(ops, sc)
    kw = dict(max_depth_error=0.01, max_reproj_error=2.0, min_num_pixels=3, want_pixel=True)
    a = ops.colmap_fuse(depths, colors, cams, sc["overlap"], **kw)
    b = ops.colmap_fuse(depths, colors, cams, sc["overlap"], **kw)
    torch.cuda.synchronize()
    assert a[0].shape[0] > 500
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_capacity_overflow_is_a_clean_error(env):
    L, ops, synthetic = env
    sc = synthetic.make_yfcc_fusion_scene(5, 24, 32, seed=2)
    depths, colors, cams, _ = _inputs(ops, sc)
    kw = dict(max_depth_error=0.01, max_reproj_error=1.0, min_num_pixels=2)
    full = ops.colmap_fuse(depths, colors, cams, sc["overlap"], **kw)
    m = full[0].shape[0]
    assert m > 50
    with pytest.raises(L.PscvError, match="capacity"):
        ops.colmap_fuse(depths, colors, cams, sc["overlap"], capacity=m - 1, **kw)
    with pytest.raises(L.PscvError, match="capacity"):
        fused = [torch.zeros(d.shape, dtype=torch.uint8, device="cuda") for d in depths]
        ops.colmap_fuse_pass(0, depths, colors, cams, sc["overlap"], fused, capacity=3, **kw)
    exact = ops.colmap_fuse(depths, colors, cams, sc["overlap"], capacity=m, **kw)
    torch.cuda.synchronize()
    for x, y in zip(full, exact):
        assert torch.equal(x, y)


def test_every_limit_raises(env):
    L, ops, synthetic = env
    sc = synthetic.make_yfcc_fusion_scene(3, 12, 16, seed=2)
    depths, colors, cams, _ = _inputs(ops, sc)
    ov = sc["overlap"]
    ok = dict(max_depth_error=0.01, max_reproj_error=1.0, min_num_pixels=2)
    bad = [dict(max_reproj_error=0.0), dict(max_reproj_error=2.5), dict(max_depth_error=0.0), dict(max_depth_error=1.0),
           dict(min_num_pixels=0), dict(max_traversal_depth=0), dict(max_num_pixels=1 + 2 * 9 - 1)]
    for b in bad:
        with pytest.raises(ValueError):
            ops.colmap_fuse(depths, colors, cams, ov, **{**ok, **b})
    ops.colmap_fuse(depths, colors, cams, ov, **{**ok, "max_num_pixels": 1 + 2 * 9})          # the bound itself is allowed
    with pytest.raises(ValueError):
        ops.colmap_fuse(depths[:1], colors[:1], cams[:1], [[]], **ok)                       # N < 2
    with pytest.raises(ValueError):
        ops.colmap_fuse(depths * 22, colors * 22, cams.repeat(22, 1), [[]] * 66, **ok)       # N > 64
    with pytest.raises(ValueError):
        ops.colmap_fuse(depths, colors, cams, [[1], [7], []], **ok)                          # overlap names a missing view
    fused = [torch.zeros(d.shape, dtype=torch.uint8, device="cuda") for d in depths]
    with pytest.raises(ValueError):
        ops.colmap_fuse_pass(1, depths, colors, cams, ov, fused, processed=[1], **ok)        # its own view processed
    # the C entry point checks its limits too
    with pytest.raises(L.PscvError, match="max_reproj_error"):
        run = ops._ColmapRun(depths, colors, cams, ov, None, None, (0.01, 1.0, 2, 100, 10000))
        run.params = (0.01, 3.0, 2, 100, 10000)
        run.run_pass(0, 0, 0)


def test_colmap_fusion_writes_what_metrics_run_reads(env, tmp_path, capsys, monkeypatch):
    """evaluation.colmap_fusion.colmap_fusion: reads <scene>/<view>_out.npz depth + probability (a missing file skips the view),
    masks like the reference, scales K to the depth map, samples colours nearest-neighbour, takes the overlap from the sparse
    model when there is one, fuses and writes Points/<model>_<nviews>/<model>_<nviews><scene>.ply, which metrics.run reads."""
    L, ops, synthetic = env
    from wild_deep_mvs_amd.evaluation import colmap_fusion as CF, metrics as M
    from wild_deep_mvs_amd.utils.point_cloud import read_ply
    V, H, W, ds = 5, 24, 32, 2
    sc = synthetic.make_yfcc_fusion_scene(V, H, W, seed=4)
    args = Namespace(model="vis", nviews=V, data_path=str(tmp_path), scene="sceneA_5", downscale=ds, colmap=False, filter=True,
                     upsample=False, prob_threshold=0.5, fusion_depth_threshold=0.01, fusion_max_reproj_error=1.0,
                     fusion_num_consistent=3, override=False, dataset="yfcc", override_fusion=True)
    folder = f"{args.model}_{args.nviews}"
    dfold = tmp_path / "IntRes" / "depthmaps" / folder / "sceneA_5"
    gfold = tmp_path / "IntRes" / "geometric_filtering" / folder / "sceneA_5"
    dfold.mkdir(parents=True)
    gfold.mkdir(parents=True)
    rng = np.random.default_rng(0)
    batches, masked, colors, Ks = [], [], [], []
    for v in range(V):
        name = f"{v:08d}"
        d = sc["depths"][v].numpy()
        h, w = d.shape
        prob = np.ones((h, w), np.float32)
        prob[2:6, 3:9] = 0.2
        geo = np.ones((h, w), bool)
        geo[:, :2] = False
        if v != 3:                                      # view 3 has no depth map: skipped
            np.savez(dfold / f"{name}_out.npz", depthmap=d, probability=prob)
            np.savez(gfold / f"{name}_out.npz", geo_mask=geo)
        img = torch.from_numpy(rng.random((1, 1, 3, h * ds, w * ds), dtype=np.float32))
        Kf = sc["K"][v].clone().double()
        Kf[:2] *= ds
        batches.append({"filename": [name], "imgs": img, "K": Kf.float()[None, None], "R": sc["R"][v][None, None],
                        "t": sc["t"][v][None, None]})
        if v != 3:
            dm = d.copy()
            dm[(prob < 0.5) | ~geo] = 0
            masked.append(dm)
            colors.append(CF.nearest_colors(img[0, 0], h, w))
            Ks.append(v)
    CF.colmap_fusion(batches, args)
    assert "all other views" in capsys.readouterr().out
    out = tmp_path / "Points" / folder / f"{folder}sceneA_5.ply"
    data = read_ply(out)
    K = sc["K"][Ks].clone().double()
    K[:, :2] = (K[:, :2] * ds) / ds
    cams = ops.geo_filter_cams(K.float(), sc["R"][Ks], sc["t"][Ks]).cuda()
    ov = [[u for u in range(4) if u != v] for v in range(4)]
    xyz, nor, rgb, view = ops.colmap_fuse([torch.from_numpy(m).cuda() for m in masked], [torch.from_numpy(c).cuda() for c in colors],
                                          cams, ov, max_depth_error=0.01, max_reproj_error=1.0, min_num_pixels=3)
    assert len(data) == xyz.shape[0] > 100
    np.testing.assert_array_equal(np.stack([data[c] for c in "xyz"], axis=1), xyz.cpu().numpy())
    np.testing.assert_array_equal(np.stack([data[c] for c in ("nx", "ny", "nz")], axis=1), nor.cpu().numpy())
    np.testing.assert_array_equal(np.stack([data[c] for c in ("red", "green", "blue")], axis=1), rgb.cpu().numpy())
    # an existing file is kept unless args.override
    stamp = out.read_bytes()
    CF.colmap_fusion(batches, args)
    assert "already done" in capsys.readouterr().out and out.read_bytes() == stamp
    # metrics.run reads it (the YFCC branch)
    monkeypatch.chdir(tmp_path)
    (tmp_path / "data" / "yfcc_subset_dataset" / "gt_resolution").mkdir(parents=True)
    (tmp_path / "data" / "yfcc_subset_dataset" / "gt_resolution" / "sceneA.txt").write_text("0.05\n")
    from wild_deep_mvs_amd.utils.point_cloud import write_point_cloud
    (tmp_path / "Points" / "gt").mkdir(parents=True)
    write_point_cloud(tmp_path / "Points" / "gt" / "sceneA_gt.ply", xyz.cpu().numpy() + 0.01, rgb.cpu().numpy())
    M.run(args)
    assert (tmp_path / "IntRes" / "chamfer" / folder / "distssceneA_5.pkl").exists()
    # under args.colmap the fusion needs COLMAP's own maps
    args.colmap, args.override = True, True
    with pytest.raises(NotImplementedError):
        CF.colmap_fusion(batches, args)
