"""GPU: what the depth-map overlap graph buys the COLMAP-style fusion, and the ``fusion_overlap`` option end to end.

The scene (tests/_covisibility_ref.py::scene_fusion) is an unordered collection: 64 ragged views around 24 x 32 on an 8 x 8 rig
spaced 1.5 apart (a view shares surface with about 11 others), shuffled so that index neighbours are not spatial neighbours, fused
with the reference configuration (max_depth_error 0.01, max_reproj_error 1, fusion_num_consistent = min_num_pixels = 3) three ways:
  (a) the scene's own lists, every other view nearest camera centre first, cut at CHECK_NUM_IMAGES = 50;
  (b) the fallback without a sparse model: the first 50 other views by index;
  (c) the lists of the depth-map covisibility at stride 4.
The numpy rules alone (tests/_colmap_fusion_ref.py::parallel_fuse with the lists of tests/_covisibility_ref.py::covisibility,
on the CPU) give
    (a) 5499 points    (b) 3768 points    (c) 5487 points
so the fallback loses 31 % of the cloud (true neighbours past index 50 never support a pixel) and (c) / (a) = 0.9978.  The GPU
run has to show points(c) >= points(a) x R with R = 0.9978 - 0.02 (the 2 % for the few borderline samples) and
points(c) > points(b)."""
from argparse import Namespace

import numpy as np
import pytest
import torch

from tests import _covisibility_ref as VR

pytestmark = pytest.mark.gpu

REF_POINTS = {"a": 5499, "b": 3768, "c": 5487}          # the numpy rules on the CPU (see above)
R = REF_POINTS["c"] / REF_POINTS["a"] - 0.02


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from wild_deep_mvs_amd import _lib as L, ops
    L.lib()
    return L, ops


def test_depth_overlap_keeps_the_cloud_the_index_fallback_loses(env):
    from wild_deep_mvs_amd.evaluation.colmap_fusion import CHECK_NUM_IMAGES
    from wild_deep_mvs_amd.utils.colmap_model import overlap_from_covisibility
    L, ops = env
    sc = VR.scene_fusion()
    V = len(sc["depths"])
    assert V == 64 and sc["perm"].tolist() != list(range(V))
    depths, colors, cams = [d.cuda() for d in sc["depths"]], [c.cuda() for c in sc["colors"]], VR.cams_of(sc).cuda()
    counts = ops.view_covisibility(depths, cams, stride=VR.FUSION_STRIDE, max_depth_error=VR.MAX_DEPTH_ERROR)
    lists = {"a": [l[:CHECK_NUM_IMAGES] for l in sc["overlap"]],
             "b": [[u for u in range(V) if u != v][:CHECK_NUM_IMAGES] for v in range(V)],
             "c": overlap_from_covisibility(counts, CHECK_NUM_IMAGES)}
    points = {k: int(ops.colmap_fuse(depths, colors, cams, ov, **VR.FUSION_KW)[0].shape[0]) for k, ov in lists.items()}
    print(f"points: {points}, reference {REF_POINTS}, mean list length (c) {np.mean([len(l) for l in lists['c']]):.1f}")
    assert points["c"] >= points["a"] * R, (points, R)
    assert points["c"] > points["b"], points
    assert points["a"] > 1000


def _loader(sc, tmp_path, folder, scene, ds=2):
    """Batches and depth / filter files shaped like the ones evaluation.colmap_fusion reads (tests/test_gpu_colmap_fusion.py),
    and the masked depth maps, colours and cameras it derives from them."""
    from wild_deep_mvs_amd.evaluation import colmap_fusion as CF
    dfold = tmp_path / "IntRes" / "depthmaps" / folder / scene
    gfold = tmp_path / "IntRes" / "geometric_filtering" / folder / scene
    dfold.mkdir(parents=True)
    gfold.mkdir(parents=True)
    rng = np.random.default_rng(0)
    batches, masked, colors = [], [], []
    for v, d in enumerate(sc["depths"]):
        name = f"{v:08d}"
        d = d.numpy()
        h, w = d.shape
        prob = np.ones((h, w), np.float32)
        prob[2:6, 3:9] = 0.2
        geo = np.ones((h, w), bool)
        geo[:, :2] = False
        np.savez(dfold / f"{name}_out.npz", depthmap=d, probability=prob)
        np.savez(gfold / f"{name}_out.npz", geo_mask=geo)
        img = torch.from_numpy(rng.random((1, 1, 3, h * ds, w * ds), dtype=np.float32))
        Kf = sc["K"][v].clone().double()
        Kf[:2] *= ds
        batches.append({"filename": [name], "imgs": img, "K": Kf.float()[None, None], "R": sc["R"][v][None, None], "t": sc["t"][v][None, None]})
        dm = d.copy()
        dm[(prob < 0.5) | ~geo] = 0
        masked.append(torch.from_numpy(dm).cuda())
        colors.append(torch.from_numpy(CF.nearest_colors(img[0, 0], h, w)).cuda())
    K = sc["K"].clone().double()
    K[:, :2] = (K[:, :2] * ds) / ds
    return batches, masked, colors, K.float()


def test_colmap_fusion_with_the_depth_overlap_and_without_the_option(env, tmp_path, capsys):
    from wild_deep_mvs_amd.evaluation import colmap_fusion as CF
    from wild_deep_mvs_amd.utils.colmap_model import overlap_from_covisibility
    from wild_deep_mvs_amd.utils.point_cloud import read_ply, write_colmap_point_cloud
    L, ops = env
    sc = VR.scene_plain()
    V = len(sc["depths"])
    args = Namespace(model="vis", nviews=V, data_path=str(tmp_path), scene="sceneA_5", downscale=2, colmap=False, filter=True,
                     upsample=False, prob_threshold=0.5, fusion_depth_threshold=0.01, fusion_max_reproj_error=1.0,
                     fusion_num_consistent=3, override=True, dataset="yfcc", override_fusion=True)
    folder = f"{args.model}_{args.nviews}"
    batches, masked, colors, K = _loader(sc, tmp_path, folder, "sceneA_5")
    cams = ops.geo_filter_cams(K, sc["R"], sc["t"]).cuda()
    kw = dict(max_depth_error=0.01, max_reproj_error=1.0, min_num_pixels=3)
    out = tmp_path / "Points" / folder / f"{folder}sceneA_5.ply"
    assert not (tmp_path / "IntRes" / "colmap_sparse").exists()

    # the option unset: the file of the code before the option, i.e. every other view by index
    CF.colmap_fusion(batches, args)
    assert "overlap from all other views (no sparse model)" in capsys.readouterr().out
    everyone = [[u for u in range(V) if u != v] for v in range(V)]
    xyz, nor, rgb, _ = ops.colmap_fuse(masked, colors, cams, everyone, **kw)
    write_colmap_point_cloud(tmp_path / "direct.ply", xyz, nor, rgb)
    assert xyz.shape[0] > 100 and out.read_bytes() == (tmp_path / "direct.ply").read_bytes()

    # "depth": the lists of the op on the same masked maps and cameras
    args.fusion_overlap = "depth"
    CF.colmap_fusion(batches, args)
    assert "overlap from depth-map covisibility (stride 4)" in capsys.readouterr().out
    lists = overlap_from_covisibility(ops.view_covisibility(masked, cams, stride=4, max_depth_error=0.01), CF.CHECK_NUM_IMAGES)
    assert all(lists) and lists != everyone
    xyz, nor, rgb, _ = ops.colmap_fuse(masked, colors, cams, lists, **kw)
    data = read_ply(out)
    assert len(data) == xyz.shape[0] > 100
    np.testing.assert_array_equal(np.stack([data[c] for c in "xyz"], axis=1), xyz.cpu().numpy())

    # the stride option reaches the op, and "sparse" without a model raises before any file is written
    args.fusion_overlap_stride = 2
    CF.colmap_fusion(batches, args)
    assert "stride 2" in capsys.readouterr().out
    args.fusion_overlap = "sparse"
    stamp = out.read_bytes()
    with pytest.raises(FileNotFoundError):
        CF.colmap_fusion(batches, args)
    assert out.read_bytes() == stamp
