"""CPU: the overlap graph from depth-map covisibility ("Overlap without a sparse model"):
``overlap_from_covisibility``, the numpy rule of tests/_covisibility_ref.py on a scene whose answer is known in closed form, the
``fusion_overlap`` option of ``evaluation.colmap_fusion.scene_overlap`` with the op replaced by the numpy rule, and the cap on the
borderline share of every scene the GPU tests compare on."""
import os
import shutil
from argparse import Namespace

import numpy as np
import pytest
import torch

from tests import _covisibility_ref as VR

HERE = os.path.dirname(os.path.abspath(__file__))


def _counts(V, pairs):
    c = np.zeros((V, V, 2), np.int64)
    for (v, u), (seen, cons) in pairs.items():
        c[v, u] = (seen, cons)
    return c


def test_overlap_lists_order_ties_truncation_share_and_empty_views():
    from wild_deep_mvs_amd.utils.colmap_model import overlap_from_counts, overlap_from_covisibility
    # view 0: 100 samples; u = 1..4 consistent 40, 70, 40, 0 (seen but never consistent); view 5 has no valid depth
    c = _counts(6, {(0, 1): (100, 40), (0, 2): (90, 70), (0, 3): (60, 40), (0, 4): (80, 0), (1, 0): (50, 50), (2, 0): (10, 1),
                    (2, 1): (20, 2), (3, 4): (7, 7), (4, 3): (9, 3)})
    lists = overlap_from_covisibility(c)
    assert lists[0] == [2, 1, 3]                        # descending, the tie 40 = 40 by index, the inconsistent view 4 left out
    assert lists[1] == [0] and lists[2] == [1, 0] and lists[3] == [4] and lists[4] == [3]
    assert lists[5] == []                               # no valid depth: an empty list
    assert overlap_from_covisibility(c, 2)[0] == [2, 1]                        # truncation
    assert overlap_from_covisibility(c, 1)[2] == [1]
    # min_share of the valid samples (view 0: 100; view 2: 20)
    assert overlap_from_covisibility(c, 50, 0.5)[0] == [2]
    assert overlap_from_covisibility(c, 50, 0.4)[0] == [2, 1, 3]               # >= : the bound itself stays
    assert overlap_from_covisibility(c, 50, 0.1)[2] == [1]
    assert overlap_from_covisibility(c, 50, 0.5)[5] == []
    # the ordering contract is overlap_from_counts's
    assert lists == overlap_from_counts(c[:, :, 1])
    assert overlap_from_covisibility(torch.from_numpy(c).to(torch.int32)) == lists
    with pytest.raises(ValueError):
        overlap_from_covisibility(c[:, :, 0])


def _hand_scene():
    """Views 0 and 1: the same camera and the same depth map (depth 2, three masked pixels).  View 2: the same centre, turned
    away.  View 3: the camera of view 0 with every depth x 1.5."""
    from wild_deep_mvs_amd import ops
    h, w = 6, 8
    K = torch.tensor([[7.0, 0.0, 3.5], [0.0, 7.0, 2.5], [0.0, 0.0, 1.0]])
    eye, away = torch.eye(3), torch.diag(torch.tensor([-1.0, 1.0, -1.0]))
    d = torch.full((h, w), 2.0)
    d[0, 0] = d[2, 4] = d[3, 3] = 0.0                   # (0, 0) and (2, 4) are samples of the stride-2 grid
    cams = ops.geo_filter_cams(K.expand(4, 3, 3).clone(), torch.stack((eye, eye, away, eye)), torch.zeros(4, 3, 1))
    return [d, d.clone(), d.clone(), d * 1.5], cams


@pytest.mark.parametrize("stride", [1, 2])
def test_reference_on_a_scene_with_a_closed_form_answer(stride):
    depths, cams = _hand_scene()
    counts, border, nvalid = VR.covisibility([x.numpy() for x in depths], cams.numpy(), stride=stride, max_depth_error=0.01)
    n = {1: 6 * 8 - 3, 2: 3 * 4 - 2}[stride]
    assert nvalid.tolist() == [n, n, n, n]
    assert counts[0, 1].tolist() == [n, n] and counts[1, 0].tolist() == [n, n]          # identical cameras see each other fully
    assert not counts[2].any() and not counts[:, 2].any()                               # the camera facing away
    assert counts[0, 3, 0] > 0 and counts[3, 0, 0] > 0 and counts[0, 3, 1] == 0 and counts[3, 0, 1] == 0    # depths x 1.5
    assert counts[0, 3, 0] == n                                                         # same camera: the same pixel, just no agreement
    assert not counts[np.arange(4), np.arange(4)].any()
    assert border.sum() == 0                            # projections land on pixel centres; ratios are 0 or 1/3, 1/2
    # the op-shaped wrapper
    like = VR.covisibility_like_op(depths, cams, stride=stride, max_depth_error=0.01)
    assert like.dtype == torch.int32 and np.array_equal(like.numpy(), counts)


def test_borderline_samples_are_counted():
    """A projection 5e-4 px from a rounding boundary and a depth ratio 5e-6 from the threshold are borderline; shifted away, not."""
    from wild_deep_mvs_amd import ops
    K = torch.tensor([[8.0, 0.0, 4.0], [0.0, 8.0, 3.0], [0.0, 0.0, 1.0]]).expand(2, 3, 3).clone()
    for shift, want in ((0.5 - 5e-4, 1), (0.25, 0)):
        t = torch.zeros(2, 3, 1)
        t[1, 0, 0] = shift * 2.0 / 8.0                  # moves every projection of depth 2 by `shift` pixels in x
        cams = ops.geo_filter_cams(K, torch.eye(3).expand(2, 3, 3).clone(), t)
        d0 = torch.zeros(6, 8)
        d0[3, 4] = 2.0
        _, border, _ = VR.covisibility([d0.numpy(), np.full((6, 8), 2.0, np.float32)], cams.numpy(), stride=1, max_depth_error=0.01)
        assert border[0, 1] == want
    cams = ops.geo_filter_cams(K, torch.eye(3).expand(2, 3, 3).clone(), torch.zeros(2, 3, 1))
    for ratio, want in ((0.01 + 5e-6, 1), (0.02, 0)):
        d0 = torch.zeros(6, 8)
        d0[3, 4] = 2.0 * (1.0 + ratio)
        counts, border, _ = VR.covisibility([d0.numpy(), np.full((6, 8), 2.0, np.float32)], cams.numpy(), stride=1, max_depth_error=0.01)
        assert counts[0, 1].tolist() == [1, 0] and border[0, 1] == want


def _args(tmp_path, **kw):
    return Namespace(data_path=str(tmp_path), scene="sceneA", fusion_depth_threshold=0.01, **kw)


def test_scene_overlap_options(tmp_path, monkeypatch):
    from wild_deep_mvs_amd import ops
    from wild_deep_mvs_amd.evaluation import colmap_fusion as CF
    from wild_deep_mvs_amd.utils.colmap_model import overlap_from_covisibility
    calls = []

    def fake(depths, cams, *, stride=4, max_depth_error):
        calls.append((stride, max_depth_error))
        return VR.covisibility_like_op(depths, cams, stride=stride, max_depth_error=max_depth_error)

    monkeypatch.setattr(ops, "view_covisibility", fake)
    names = [f"{k:08d}" for k in range(4)]
    everyone = [[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2]]
    sc = VR.scene_plain()
    depths, cams = sc["depths"][:4], VR.cams_of(sc)[:4]
    # no sparse model
    assert CF.scene_overlap(_args(tmp_path), names) == (everyone, "all other views (no sparse model)")             # today's
    assert CF.scene_overlap(_args(tmp_path, fusion_overlap="auto"), names, depths, cams)[0] == everyone
    lists, source = CF.scene_overlap(_args(tmp_path, fusion_overlap="all"), names)
    assert lists == everyone and source == "all other views"
    with pytest.raises(FileNotFoundError, match="sparse"):
        CF.scene_overlap(_args(tmp_path, fusion_overlap="sparse"), names)
    with pytest.raises(ValueError, match="fusion_overlap"):
        CF.scene_overlap(_args(tmp_path, fusion_overlap="dense"), names)
    assert calls == []
    # "depth": the lists of the (patched) counts, with the fusion's depth threshold and the stride option
    want = lambda stride: overlap_from_covisibility(VR.covisibility_like_op(depths, cams, stride=stride, max_depth_error=0.01), 50)
    lists, source = CF.scene_overlap(_args(tmp_path, fusion_overlap="depth"), names, depths, cams)
    assert lists == want(4) and calls == [(4, 0.01)] and "depth" in source and "stride 4" in source
    assert all(lists) and lists != everyone             # ordered by agreement, not by index
    lists, source = CF.scene_overlap(_args(tmp_path, fusion_overlap="depth", fusion_overlap_stride=2), names, depths, cams)
    assert lists == want(2) and calls[-1] == (2, 0.01) and "stride 2" in source
    with pytest.raises(ValueError, match="depth"):
        CF.scene_overlap(_args(tmp_path, fusion_overlap="depth"), names)                 # nothing to count on
    # with the sparse model of tests/golden/colmap_tiny
    sparse = tmp_path / "IntRes" / "colmap_sparse" / "sceneA"
    shutil.copytree(os.path.join(HERE, "golden", "colmap_tiny"), sparse)
    model = [[1, 2, 3], [0, 2, 3], [0, 1, 3], [2, 0, 1]]
    assert CF.scene_overlap(_args(tmp_path), names) == (model, f"sparse model {sparse}")                           # today's
    assert CF.scene_overlap(_args(tmp_path, fusion_overlap="sparse"), names) == (model, f"sparse model {sparse}")
    assert CF.scene_overlap(_args(tmp_path, fusion_overlap="all"), names) == (everyone, "all other views")
    assert CF.scene_overlap(_args(tmp_path, fusion_overlap="depth"), names, depths, cams)[0] == want(4)


@pytest.mark.parametrize("case", list(VR.GPU_CASES))
def test_borderline_share_of_the_gpu_scenes_is_at_most_one_percent(case):
    """The GPU tests allow |gpu - reference| <= the pair's borderline count; this cap keeps that allowance from hiding a failure."""
    make, stride = VR.GPU_CASES[case]
    sc = make()
    _, border, nvalid = VR.covisibility([d.numpy() for d in sc["depths"]], VR.cams_of(sc).numpy(), stride=stride,
                                        max_depth_error=VR.MAX_DEPTH_ERROR)
    pairs = int(nvalid.sum()) * (len(nvalid) - 1)
    assert pairs > 0 and border.sum() <= 0.01 * pairs, f"{case}: {int(border.sum())} borderline of {pairs} (sample, target) pairs"


def test_permuted_scene_is_the_grid_scene_renumbered():
    from wild_deep_mvs_amd import synthetic
    a = synthetic.make_yfcc_fusion_scene(9, 12, 16, seed=3)
    b = synthetic.make_permuted_yfcc_fusion_scene(9, 12, 16, seed=3, perm_seed=1)
    perm = b["perm"]
    assert sorted(perm.tolist()) == list(range(9)) and perm.tolist() != list(range(9))
    for k, p in enumerate(perm):
        assert torch.equal(b["depths"][k], a["depths"][p]) and torch.equal(b["K"][k], a["K"][p]) and torch.equal(b["t"][k], a["t"][p])
        assert [int(perm[u]) for u in b["overlap"][k]] == a["overlap"][p]
