"""GPU: COLMAP-style stereo fusion with normal maps (pscv_colmap_fuse_pass_normals, the NORMALS = true kernels of
csrc/colmap_fusion.hip) against the numpy rule of tests/_colmap_fusion_normals_ref.py, bit for bit: after every pass the fused
masks and the point count match exactly and xyz, normal, rgb and the seed pixels are equal as 32-bit words.  Each case first
shows, from the numpy side, that its scene exercises the normal test.  Also: the normal-free call is unchanged, determinism,
every new limit, the capacity check, and the COLMAP baseline end to end (depthmap_colmap -> colmap_fusion under args.colmap ->
metrics.run) with its measured accuracy.

The measured accuracy of the end-to-end case is in the docstring of ``test_colmap_baseline_end_to_end`` and in the table of
INTEGRATION.md section 2g."""
from argparse import Namespace

import numpy as np
import pytest
import torch

from tests import _colmap_fusion_normals_ref as NR
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
    return ([d.cuda() for d in sc["depths"]], [c.cuda() for c in sc["colors"]], [n.cuda() for n in sc["normals"]], cams.cuda(),
            cams.numpy())


CASES = {  # name: (V, H, W, scene options, fusion options)
    "n2_e10": (2, 24, 32, {}, {"max_reproj_error": 1.0, "min_num_pixels": 2, "max_normal_error": 10.0}),
    "n5_r1_e10": (5, 24, 32, {}, {"max_reproj_error": 1.0, "min_num_pixels": 3, "max_normal_error": 10.0}),
    "n5_r2_e30": (5, 24, 32, {"rot_deg": 45.0}, {"max_reproj_error": 2.0, "min_num_pixels": 3, "max_normal_error": 30.0}),
    "n10_knn_r15_e10": (10, 20, 28, {"overlap": "knn", "k_overlap": 3},
                        {"max_reproj_error": 1.5, "min_num_pixels": 3, "max_normal_error": 10.0}),
    "n10_chain_td2_e10": (10, 20, 28, {"overlap": "chain"},
                          {"max_reproj_error": 1.0, "min_num_pixels": 2, "max_traversal_depth": 2, "max_normal_error": 10.0}),
    "n20_e10": (20, 16, 20, {}, {"max_reproj_error": 1.0, "min_num_pixels": 3, "max_normal_error": 10.0}),
}


@pytest.mark.parametrize("case", list(CASES))
def test_each_pass_matches_the_rule(env, case):
    L, ops, synthetic = env
    V, H, W, sopt, fopt = CASES[case]
    sc = synthetic.make_normal_fusion_scene(V, H, W, seed=3, **sopt)
    depths, colors, normals, cams, cams_np = _inputs(ops, sc)
    kw = dict(max_depth_error=0.01, **fopt)
    d_np, c_np, n_np = ([x.numpy() for x in sc[k]] for k in ("depths", "colors", "normals"))
    # the scene must make the normal test bite (numpy side): over the whole run at least 5 % of the pairs that pass depth and
    # reprojection fail the normal test, and the point count differs from the count with the test off
    *_, passes_on = NR.parallel_fuse(d_np, c_np, n_np, cams_np, sc["overlap"], **kw)
    *_, passes_off = NR.parallel_fuse(d_np, c_np, n_np, cams_np, sc["overlap"], **{**kw, "max_normal_error": 180.0})
    tested, rejected = sum(p["tested"] for _, p in passes_on), sum(p["rejected"] for _, p in passes_on)
    count_on, count_off = sum(len(p["xyz"]) for _, p in passes_on), sum(len(p["xyz"]) for _, p in passes_off)
    print(f"{case}: {rejected} of {tested} tested pairs fail the normal test ({rejected / max(tested, 1):.3f}); points {count_on} "
          f"at {fopt['max_normal_error']} degrees, {count_off} at 180")
    assert tested > 0 and rejected >= 0.05 * tested, (rejected, tested)
    assert count_on != count_off, (count_on, count_off)
    assert sum(p["rejected"] for _, p in passes_off) == 0

    fused = [torch.zeros(d.shape, dtype=torch.uint8, device="cuda") for d in depths]
    processed, total, outs = [], 0, []
    order = ops.find_next_image_order(ops.colmap_overlap_lists(sc["overlap"], V))
    assert order == [v for v, _ in passes_on]
    for v in order:
        before = [f.cpu().numpy() for f in fused]
        want = NR.parallel_pass(v, d_np, c_np, n_np, cams_np, sc["overlap"], [u in processed for u in range(V)], before, **kw)
        assert want["margin"] >= 1e-9, f"pass {v}: a decision lies {want['margin']:.2e} from its threshold"
        xyz, nor, rgb, pix = ops.colmap_fuse_pass(v, depths, colors, cams, sc["overlap"], fused, processed=processed,
                                                  normals=normals, **kw)
        torch.cuda.synchronize()
        for u in range(V):
            np.testing.assert_array_equal(fused[u].cpu().numpy(), want["fused"][u], err_msg=f"pass {v}: fused mask of view {u}")
        assert xyz.shape[0] == len(want["xyz"]), f"pass {v}"
        np.testing.assert_array_equal(pix.cpu().numpy(), want["pixel"])
        np.testing.assert_array_equal(xyz.cpu().numpy().view(np.uint32), want["xyz"].view(np.uint32))
        np.testing.assert_array_equal(nor.cpu().numpy().view(np.uint32), want["normal"].view(np.uint32))
        np.testing.assert_array_equal(rgb.cpu().numpy(), want["rgb"])
        total += xyz.shape[0]
        outs.append((xyz.cpu(), nor.cpu()))
        processed.append(v)
    assert total == count_on > 20
    # the whole run is the passes in order
    xyz, nor, rgb, view = ops.colmap_fuse(depths, colors, cams, sc["overlap"], normals=normals, **kw)
    assert torch.equal(xyz.cpu(), torch.cat([o[0] for o in outs])) and torch.equal(nor.cpu(), torch.cat([o[1] for o in outs]))


def test_without_normals_the_call_is_what_it_was(env):
    """normals=None goes to pscv_colmap_fuse_pass: the numpy rule of _colmap_fusion_ref, bit for bit (one case of
    test_gpu_colmap_fusion.py, repeated here on purpose)."""
    L, ops, synthetic = env
    sc = synthetic.make_yfcc_fusion_scene(5, 24, 32, seed=3)
    cams = ops.geo_filter_cams(sc["K"], sc["R"], sc["t"])
    kw = dict(max_depth_error=0.01, max_reproj_error=1.0, min_num_pixels=3)
    wx, wn, wc, wv, margin, _ = CR.parallel_fuse([d.numpy() for d in sc["depths"]], [c.numpy() for c in sc["colors"]], cams.numpy(),
                                                 sc["overlap"], **kw)
    assert margin >= 1e-9
    xyz, nor, rgb, view = ops.colmap_fuse([d.cuda() for d in sc["depths"]], [c.cuda() for c in sc["colors"]], cams.cuda(),
                                          sc["overlap"], normals=None, max_normal_error=None, **kw)
    torch.cuda.synchronize()
    assert xyz.shape[0] == len(wx) > 100
    np.testing.assert_array_equal(xyz.cpu().numpy().view(np.uint32), wx.view(np.uint32))
    np.testing.assert_array_equal(nor.cpu().numpy().view(np.uint32), wn.view(np.uint32))
    np.testing.assert_array_equal(rgb.cpu().numpy(), wc)
    np.testing.assert_array_equal(view.cpu().numpy(), wv)


def test_fusion_with_normals_is_deterministic(env):
    L, ops, synthetic = env
    sc = synthetic.make_normal_fusion_scene(10, 48, 64, seed=7)
    depths, colors, normals, cams, _ = _inputs(ops, sc)
    kw = dict(max_depth_error=0.01, max_reproj_error=2.0, min_num_pixels=3, want_pixel=True, normals=normals, max_normal_error=10.0)
    a = ops.colmap_fuse(depths, colors, cams, sc["overlap"], **kw)
    b = ops.colmap_fuse(depths, colors, cams, sc["overlap"], **kw)
    torch.cuda.synchronize()
    assert a[0].shape[0] > 500
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_capacity_overflow_is_a_clean_error(env):
    L, ops, synthetic = env
    sc = synthetic.make_normal_fusion_scene(5, 24, 32, seed=2)
    depths, colors, normals, cams, _ = _inputs(ops, sc)
    kw = dict(max_depth_error=0.01, max_reproj_error=1.0, min_num_pixels=2, normals=normals, max_normal_error=10.0)
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


def test_every_new_limit_raises(env):
    L, ops, synthetic = env
    sc = synthetic.make_normal_fusion_scene(3, 12, 16, seed=2)
    depths, colors, normals, cams, _ = _inputs(ops, sc)
    ov = sc["overlap"]
    ok = dict(max_depth_error=0.01, max_reproj_error=1.0, min_num_pixels=2)
    ops.colmap_fuse(depths, colors, cams, ov, normals=normals, max_normal_error=180.0, **ok)          # the bound itself is allowed
    for bad in (0.0, -1.0, 181.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="max_normal_error"):
            ops.colmap_fuse(depths, colors, cams, ov, normals=normals, max_normal_error=bad, **ok)
    with pytest.raises(ValueError, match="go together"):
        ops.colmap_fuse(depths, colors, cams, ov, normals=normals, **ok)
    with pytest.raises(ValueError, match="go together"):
        ops.colmap_fuse(depths, colors, cams, ov, max_normal_error=10.0, **ok)
    fused = [torch.zeros(d.shape, dtype=torch.uint8, device="cuda") for d in depths]
    with pytest.raises(ValueError, match="go together"):
        ops.colmap_fuse_pass(0, depths, colors, cams, ov, fused, normals=normals, **ok)
    wrong = [
        normals[:2],                                                                     # one map short
        [normals[0], normals[1], normals[2][:-1].contiguous()],                          # shape
        [normals[0], normals[1][..., :2].contiguous(), normals[2]],                      # two channels
        [normals[0].double(), normals[1], normals[2]],                                   # dtype
        [normals[0], normals[1], normals[2].permute(1, 0, 2)],                           # shape (transposed, not contiguous)
    ]
    for w in wrong:
        with pytest.raises(ValueError):
            ops.colmap_fuse(depths, colors, cams, ov, normals=w, max_normal_error=10.0, **ok)
    with pytest.raises((ValueError, RuntimeError)):                                      # device
        ops.colmap_fuse(depths, colors, cams, ov, normals=[normals[0].cpu(), normals[1], normals[2]], max_normal_error=10.0, **ok)
    sq = torch.zeros((12, 12, 3), device="cuda").permute(1, 0, 2)                        # right shape, not contiguous
    with pytest.raises(ValueError, match="contiguous"):
        ops.colmap_fuse([torch.ones(12, 12, device="cuda")] * 2, [torch.zeros(12, 12, 3, dtype=torch.uint8, device="cuda")] * 2,
                        cams[:2].contiguous(), [[1], [0]], normals=[sq, sq], max_normal_error=10.0, **ok)
    # the C entry point checks its limits too
    for bad in (0.0, 181.0, float("nan")):
        with pytest.raises(L.PscvError, match="max_normal_error"):
            run = ops._ColmapRun(depths, colors, cams, ov, None, None, (0.01, 1.0, 2, 100, 10000), normals=normals, max_normal_error=10.0)
            run.max_normal_error = bad
            run.run_pass(0, 0, 0)
    with pytest.raises(L.PscvError, match="max_reproj_error"):
        run = ops._ColmapRun(depths, colors, cams, ov, None, None, (0.01, 1.0, 2, 100, 10000), normals=normals, max_normal_error=10.0)
        run.params = (0.01, 3.0, 2, 100, 10000)
        run.run_pass(0, 0, 0)
    with pytest.raises(L.PscvError, match="null normal map"):
        import ctypes as C
        run = ops._ColmapRun(depths, colors, cams, ov, None, None, (0.01, 1.0, 2, 100, 10000), normals=normals, max_normal_error=10.0)
        run.nptr = (C.c_void_p * 3)(normals[0].data_ptr(), None, normals[2].data_ptr())
        run.run_pass(0, 0, 0)


def test_colmap_baseline_end_to_end(env, tmp_path, capsys, monkeypatch):
    """depthmap_colmap then colmap_fusion under args.colmap (model None, no IntRes/depthmaps folder) on a 5-view 96 x 128
    ``make_patch_match_scene``: the fallback folder is named, the .ply equals ops.colmap_fuse with the written normal maps at 10
    degrees bit for bit, every normal is unit, metrics.run reads the file.  Accuracy is measured here, not fixed:
      (a) the median angle between a fused normal and the true world normal at its seed pixel is at most 1.10 x the median normal
          error of the input geometric maps over their kept pixels (a fused normal is a median of >= 3 normals within 10 degrees;
          the 10 % is for the different pixel population);
      (b) the share of fused points within 1 % of the true depth along the seed's ray is not lower than with the test off
          (max_normal_error = 180) on the same maps: the test only removes candidates, and the run is deterministic.
    Measured on one MI355X (6669 points at 10 degrees, 8064 at 180): (a) fused 1.56 deg against 3.90 deg of the inputs; (b) 0.959 at
    10 degrees against 0.929 at 180."""
    L, ops, synthetic = env
    from wild_deep_mvs_amd.evaluation import colmap_fusion as CF, metrics as M
    from wild_deep_mvs_amd.evaluation.colmap_stereo import depthmap_colmap
    from wild_deep_mvs_amd.utils.colmap_array import read_array
    from wild_deep_mvs_amd.utils.point_cloud import read_ply, write_point_cloud
    V, H, W = 5, 96, 128
    sc = synthetic.make_patch_match_scene(V, H, W)
    batches = synthetic.patch_match_batches(sc)
    args = Namespace(model=None, nviews=V, data_path=str(tmp_path), scene="sceneC_5", downscale=1, colmap=True, filter=False,
                     upsample=False, prob_threshold=0.5, fusion_depth_threshold=0.01, fusion_max_reproj_error=1.0,
                     fusion_num_consistent=3, override=False, dataset="yfcc", override_fusion=True)
    with pytest.raises(NotImplementedError, match="depthmap_colmap"):        # nothing to fuse before the stereo has run
        CF.colmap_fusion(batches, args)
    depthmap_colmap(batches, args)
    capsys.readouterr()
    CF.colmap_fusion(batches, args)
    direct = tmp_path / "IntRes" / "direct_depthmaps" / "colmap" / "sceneC_5"
    assert str(direct) in capsys.readouterr().out
    out = tmp_path / "Points" / f"None_{V}" / f"None_{V}sceneC_5.ply"
    data = read_ply(out)

    # the same maps through ops.colmap_fuse
    stereo = tmp_path / "IntRes" / "colmap_dense" / "sceneC_5" / "stereo"
    views = [CF.view_inputs(args, b, direct / f"{b['filename'][0]}_out.npz") for b in batches]
    nmaps = [read_array(stereo / "normal_maps" / f"{b['filename'][0]}.jpg.geometric.bin") for b in batches]
    dmaps, colors, K, R, t = zip(*views)
    cams = ops.geo_filter_cams(torch.stack(K), torch.stack(R), torch.stack(t)).cuda()
    ov, _ = CF.scene_overlap(args, [b["filename"][0] for b in batches])
    run = lambda err: ops.colmap_fuse([torch.from_numpy(d).cuda() for d in dmaps], [torch.from_numpy(c).cuda() for c in colors], cams,
                                      ov, max_depth_error=0.01, max_reproj_error=1.0, min_num_pixels=3, want_pixel=True,
                                      normals=[torch.from_numpy(n).cuda() for n in nmaps], max_normal_error=err)
    xyz, nor, rgb, view, pixel = (x.cpu().numpy() for x in run(10.0))
    assert len(data) == xyz.shape[0] > 1000
    np.testing.assert_array_equal(np.stack([data[c] for c in "xyz"], axis=1).view(np.uint32), xyz.view(np.uint32))
    np.testing.assert_array_equal(np.stack([data[c] for c in ("nx", "ny", "nz")], axis=1).view(np.uint32), nor.view(np.uint32))
    np.testing.assert_array_equal(np.stack([data[c] for c in ("red", "green", "blue")], axis=1), rgb)
    np.testing.assert_allclose(np.linalg.norm(nor.astype(np.float64), axis=1), 1.0, rtol=0, atol=1e-6)

    # accuracy, measured
    Rn, tn, Kn = sc["R"].numpy().astype(np.float64), sc["t"].numpy().astype(np.float64), sc["K"].numpy().astype(np.float64)
    gt_world = np.einsum("vji,vhwj->vhwi", Rn, sc["normal"].numpy().astype(np.float64)).reshape(V, H * W, 3)
    gt_depth = sc["depth"].numpy().astype(np.float64).reshape(V, H * W)
    angle = lambda a, b: np.degrees(np.arccos(np.clip((a * b).sum(-1), -1.0, 1.0)))

    def measures(xyz, nor, view, pixel):
        a = angle(nor.astype(np.float64), gt_world[view, pixel])
        z = (np.einsum("nij,nj->ni", Rn[view], xyz.astype(np.float64)) + tn[view, :, 0])[:, 2]
        return float(np.median(a)), float((np.abs(z - gt_depth[view, pixel]) <= 0.01 * gt_depth[view, pixel]).mean())

    in_err = []
    for v in range(V):
        kept = dmaps[v].reshape(-1) > 0
        w = nmaps[v].reshape(-1, 3).astype(np.float64) @ Rn[v]               # R^T n of the input map
        in_err.append(angle(w[kept], gt_world[v][kept]))
    in_med = float(np.median(np.concatenate(in_err)))
    fused_med, share_10 = measures(xyz, nor, view, pixel)
    x180, n180, _, v180, p180 = (x.cpu().numpy() for x in run(180.0))
    _, share_180 = measures(x180, n180, v180, p180)
    with capsys.disabled():
        print(f"\n[colmap baseline] {V} views {H}x{W}: {xyz.shape[0]} points at 10 degrees, {x180.shape[0]} at 180; median normal error: fused "
              f"{fused_med:.3f} deg, input geometric maps {in_med:.3f} deg; within 1 % of the true depth: {share_10:.4f} at 10 degrees, "
              f"{share_180:.4f} at 180")
    assert fused_med <= 1.10 * in_med, (fused_med, in_med)
    assert share_10 >= share_180, (share_10, share_180)

    # an existing file is kept unless args.override
    stamp = out.read_bytes()
    CF.colmap_fusion(batches, args)
    assert "already done" in capsys.readouterr().out and out.read_bytes() == stamp
    # metrics.run reads it (the YFCC branch)
    monkeypatch.chdir(tmp_path)
    (tmp_path / "data" / "yfcc_subset_dataset" / "gt_resolution").mkdir(parents=True)
    (tmp_path / "data" / "yfcc_subset_dataset" / "gt_resolution" / "sceneC.txt").write_text("0.05\n")
    (tmp_path / "Points" / "gt").mkdir(parents=True)
    write_point_cloud(tmp_path / "Points" / "gt" / "sceneC_gt.ply", xyz + 0.01, rgb)
    M.run(args)
    assert (tmp_path / "IntRes" / "chamfer" / f"None_{V}" / "distssceneC_5.pkl").exists()
