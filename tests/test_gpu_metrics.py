"""GPU: the point-cloud metrics (csrc/point_metrics.hip behind ops.radius_downsample / ops.nn_dist and
evaluation/metrics.py) against the reference's own results (tests/golden/metrics_tiny.npz) and the numpy rules of
tests/_metrics_ref.py: kept masks bit for bit, bounded distances to rtol 1e-12 with the inf / maxdist patterns exact, the
run() mirror's pickles, determinism and a 2 M x 0.5 M case checked on sampled queries.

Kernel and rules compute the same fp64 sums from the same float32 coordinates, so they agree everywhere; a disagreement is
tolerated only on `fragile` entries, whose squared distance lies within 1e-9 (relative) of the bound, and those must be rare."""
import os
import pickle
from argparse import Namespace
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import _metrics_ref as MR

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from wild_deep_mvs_amd import _lib as L, ops, synthetic
    from wild_deep_mvs_amd.evaluation import metrics as M
    L.lib()
    return L, ops, synthetic, M


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(HERE, "golden", "metrics_tiny.npz")))


def _g(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _rank(perm):
    r = np.empty(len(perm), dtype=np.int32)
    r[perm] = np.arange(len(perm), dtype=np.int32)
    return torch.from_numpy(r).cuda()


def _agree(got, want, fragile=None, rtol=1e-12):
    """Same inf pattern, same exact-`maxdist` pattern, values to rtol; mismatches only on rare fragile entries."""
    assert got.shape == want.shape and got.dtype == np.float64
    bad = (np.isinf(got) != np.isinf(want))
    fin = np.isfinite(got) & np.isfinite(want)
    bad |= fin & ~np.isclose(got, want, rtol=rtol, atol=0.0)
    if fragile is None:
        fragile = np.zeros(got.shape, dtype=bool)
    assert not (bad & ~fragile).any(), f"{int((bad & ~fragile).sum())} mismatches, e.g. {np.nonzero(bad & ~fragile)[0][:5]}"
    assert fragile.sum() <= max(2, got.size // 1000)


# ---------------------------------------------------------------------------------------------------------------------------
# kept masks
def test_reduce_pts_matches_the_reference_golden(env, gold):
    L, ops, synthetic, M = env
    np.random.seed(int(gold["seed"]))
    kept, mask = M.reduce_pts(gold["pred"], float(gold["reduce_dst"]))
    assert mask.dtype == bool
    np.testing.assert_array_equal(mask, gold["reduce_mask"])
    np.testing.assert_array_equal(kept, gold["pred"][gold["reduce_mask"]])
    _, m2, rounds = ops.radius_downsample(_g(gold["pred"]), 0.2, _rank(gold["reduce_perm"]))
    np.testing.assert_array_equal(m2.cpu().numpy(), gold["reduce_mask"])
    assert 1 <= rounds <= 40


def _cloud(kind, rng):
    if kind == "uniform":
        return rng.uniform(0, 4.0, (3000, 3)), 0.5
    if kind == "clustered":
        c = rng.uniform(0, 20, (40, 3))
        return c[rng.integers(0, 40, 3000)] + rng.normal(0, 0.3, (3000, 3)), 0.25
    if kind == "duplicates":
        base = rng.uniform(0, 5, (600, 3))
        return np.concatenate((base, base, base[:300], rng.uniform(0, 5, (200, 3)))), 0.2
    if kind == "all_within":
        return rng.uniform(0, 0.1, (500, 3)), 1.0
    if kind == "one":
        return rng.uniform(0, 1, (1, 3)), 0.2
    if kind == "two_near":
        return np.array([[0.0, 0.0, 0.0], [0.1, 0.0, 0.0]]), 0.2
    if kind == "two_at_dst":
        return np.array([[1.0, 1.0, 1.0], [1.5, 1.0, 1.0]]), 0.5           # exactly dst apart: neighbours (inclusive)
    raise KeyError(kind)


KINDS = ["uniform", "clustered", "duplicates", "all_within", "one", "two_near", "two_at_dst"]


@pytest.mark.parametrize("kind", KINDS)
def test_kept_mask_matches_the_greedy_rule(env, kind):
    L, ops, synthetic, M = env
    rng = np.random.default_rng(KINDS.index(kind))
    pts, dst = _cloud(kind, rng)
    pts = pts.astype(np.float32)
    perm = rng.permutation(pts.shape[0])
    nbrs, fragile = MR.neighbours(pts, dst)
    want = MR.greedy_mis(nbrs, perm)
    kept, mask, rounds = ops.radius_downsample(_g(pts), dst, _rank(perm))
    mask = mask.cpu().numpy()
    if not fragile:
        np.testing.assert_array_equal(mask, want)
    else:
        assert kind == "two_at_dst" and np.array_equal(mask, want)
    np.testing.assert_array_equal(kept.cpu().numpy(), pts[mask])
    if kind == "all_within":
        assert mask.sum() == 1 and mask[perm[0]]


def test_radius_downsample_rejects_bad_input(env):
    L, ops, synthetic, M = env
    pts = _g(np.zeros((4, 3)))
    with pytest.raises(ValueError, match="permutation"):
        ops.radius_downsample(pts, 0.1, torch.zeros(4, dtype=torch.int32, device="cuda"))
    with pytest.raises(RuntimeError, match="CPU"):
        ops.radius_downsample(pts.cpu(), 0.1, torch.arange(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="float32"):
        M.reduce_pts(np.zeros((4, 3)), 0.1)


# ---------------------------------------------------------------------------------------------------------------------------
# bounded nearest neighbour
def test_chamfer_functions_match_the_reference_golden(env, gold):
    L, ops, synthetic, M = env
    _agree(M.chamfer_imw(gold["small_from"], gold["small_to"], maxdist=float(gold["imw_maxdist"])), gold["imw_dist"])
    _agree(M.chamfer(gold["gt"], gold["pred"], gold["bb"], 60), gold["chamfer_gt_to_pred"])
    got = M.chamfer(gold["pred"], gold["gt"], gold["bb"], 60)
    _agree(got, gold["chamfer_pred_to_gt"])
    np.testing.assert_array_equal(got == 60, gold["chamfer_pred_to_gt"] == 60)


def _edge_cases(rng):
    """Targets, and queries placed exactly at maxdist (0.5) of a target, at 0 and just inside / outside."""
    t = rng.uniform(0, 8, (800, 3)).astype(np.float32)
    t[:4] = [[20, 20, 20], [30, 20, 20], [20, 30, 20], [20, 20, 30]]
    q = rng.uniform(-1, 9, (1500, 3)).astype(np.float32)
    q[:8] = [[20.5, 20, 20], [20, 20.5, 20], [20, 20, 20.5], [30, 20, 20], [20.25, 20.25, 20], [29.5, 20, 20], [25, 25, 25],
             [100, -100, 5]]
    q[8] = [np.nextafter(np.float32(20.5), np.float32(0)), 20, 20]      # just inside
    return q, t


def test_nn_dist_imw_mode_matches_brute_force(env):
    L, ops, synthetic, M = env
    rng = np.random.default_rng(5)
    q, t = _edge_cases(rng)
    for maxdist in (0.5, 0.37, 3.0, np.inf):
        want, fragile = MR.nn_bounded(q, t, maxdist)
        got = ops.nn_dist(_g(q), _g(t), maxdist).cpu().numpy()
        if maxdist == 0.5:
            assert np.isinf(got[:3]).all() and got[3] == 0.0 and np.isfinite(got[4]) and np.isinf(got[5:8]).all() and np.isfinite(got[8])
            _agree(got, want)                                     # the placed points are exact: no exclusions
        else:
            _agree(got, want, fragile)
    # fine cells forced small and large: same answers
    want, fragile = MR.nn_bounded(q, t, 3.0)
    for fc in (0.01, 2.9):
        _agree(ops.nn_dist(_g(q), _g(t), 3.0, fine_cell=fc).cpu().numpy(), want, fragile)


def test_nn_dist_empty_target_and_all_outliers(env):
    L, ops, synthetic, M = env
    rng = np.random.default_rng(6)
    q = rng.uniform(0, 10, (300, 3)).astype(np.float32)
    empty = np.zeros((0, 3), dtype=np.float32)
    assert np.isinf(ops.nn_dist(_g(q), _g(empty), 1.0).cpu().numpy()).all()
    bb = np.array([[0.0, 0.0, 0.0], [10.0, 10.0, 10.0]])
    d = ops.nn_dist(_g(q), _g(empty), 5.0, bb=bb).cpu().numpy()
    np.testing.assert_array_equal(d, MR.chamfer_blocked(q, empty, bb, 5.0)[0])
    assert (d == 5.0).all()
    far = rng.uniform(100, 110, (400, 3)).astype(np.float32)
    assert np.isinf(ops.nn_dist(_g(q), _g(far), 50.0).cpu().numpy()).all()
    assert ops.nn_dist(_g(empty), _g(far), 1.0).shape == (0,)


def test_nn_dist_dtu_mode_matches_the_blocked_rule(env):
    L, ops, synthetic, M = env
    rng = np.random.default_rng(7)
    bb = np.array([[-10.0, -12.5, -7.25], [170.0, 130.0, 95.0]])
    md = 60.0
    t = rng.uniform([-30, -30, -30], [200, 160, 120], (3000, 3))
    t = t[~((t[:, 0] > 80) & (t[:, 1] > 60))]                         # a corner without targets: empty expanded boxes
    q = rng.uniform([-40, -40, -40], [210, 170, 130], (4000, 3))
    faces = bb[0] + md * rng.integers(0, 4, (600, 3))                 # on cell faces of the lattice, in one or more axes
    q[:600] = np.where(rng.random((600, 3)) < 0.5, faces, q[:600])
    q[600:700, 0] = bb[0, 0] + md * (np.floor((bb[1, 0] - bb[0, 0]) / md) + 1)     # just past the last cell
    t, q = t.astype(np.float32), q.astype(np.float32)
    want, fragile = MR.chamfer_blocked(q, t, bb, md)
    got = ops.nn_dist(_g(q), _g(t), md, bb=bb).cpu().numpy()
    _agree(got, want, fragile)
    np.testing.assert_array_equal(got == md, want == md)
    assert (want == md).sum() > 100 and np.isinf(want).any() and np.isfinite(want).sum() > 1000
    # integer maxdist as eval_dtu passes it, and the same through metrics.chamfer
    np.testing.assert_array_equal(M.chamfer(q, t, bb, 60), got)


# ---------------------------------------------------------------------------------------------------------------------------
# pickles
def _write_cloud(path, pts):
    from wild_deep_mvs_amd.utils.point_cloud import write_point_cloud
    path.parent.mkdir(parents=True, exist_ok=True)
    write_point_cloud(path, pts, np.zeros(pts.shape, dtype=np.uint8))


def test_run_dtu_writes_the_golden_pickle(env, gold, tmp_path, monkeypatch):
    L, ops, synthetic, M = env
    args = Namespace(dataset="dtu", model="mvsnet", nviews=3, scene="scan1", data_path=str(tmp_path), chunked_eval=False)
    _write_cloud(tmp_path / "Points" / "mvsnet_3" / "mvsnet_3scan1.ply", gold["pred"])
    monkeypatch.setattr(M, "load_gt", lambda scene, path: (gold["gt"], gold["obsmask"], gold["bb"], gold["res"], gold["plane"]))
    np.random.seed(int(gold["seed"]))
    M.run(args)
    with open(tmp_path / "IntRes" / "chamfer" / "mvsnet_3" / "distsscan1.pkl", "rb") as fh:
        got = pickle.load(fh)
    assert set(got) == {"margin", "maxdist", "abovePlane", "validMask", "dist_gtToPred", "dist_predToGt"}
    assert got["margin"] == 10 and got["maxdist"] == 60
    for k in ("abovePlane", "validMask"):
        assert got[k].dtype == gold[f"dtu_{k}"].dtype and got[k].shape == gold[f"dtu_{k}"].shape
        np.testing.assert_array_equal(got[k], gold[f"dtu_{k}"])
    for k in ("dist_gtToPred", "dist_predToGt"):
        _agree(got[k], gold[f"dtu_{k}"])
    M.run(args)                                                       # already computed: no work, no change


def test_run_yfcc_writes_the_golden_pickle(env, gold, tmp_path, monkeypatch):
    L, ops, synthetic, M = env
    monkeypatch.chdir(tmp_path)
    (tmp_path / "data" / "yfcc_subset_dataset" / "gt_resolution").mkdir(parents=True)
    (tmp_path / "data" / "yfcc_subset_dataset" / "gt_resolution" / "sceneA.txt").write_text("0.05\n")
    _write_cloud(tmp_path / "Points" / "gt" / "sceneA_gt.ply", gold["small_to"])
    _write_cloud(tmp_path / "Points" / "vis_5" / "vis_5sceneA_3.ply", gold["small_from"])
    args = Namespace(dataset="yfcc", model="vis", nviews=5, scene="sceneA_3", data_path=str(tmp_path), override_fusion=True)
    M.run(args)
    with open(tmp_path / "IntRes" / "chamfer" / "vis_5" / "distssceneA_3.pkl", "rb") as fh:
        got = pickle.load(fh)
    assert set(got) == {"dist_gtToPred", "dist_predToGt"}
    for k in got:
        _agree(got[k], gold[f"yfcc_{k}"])


# ---------------------------------------------------------------------------------------------------------------------------
# determinism and scale
def test_two_runs_are_bit_identical(env):
    L, ops, synthetic, M = env
    sc = synthetic.make_point_cloud_scene(300_000, 100_000, seed=3)
    p, t = _g(sc["pred"]), _g(sc["gt"])
    rank = _rank(np.random.default_rng(0).permutation(p.shape[0]))
    a = ops.radius_downsample(p, 0.2, rank)[1].cpu().numpy()
    b = ops.radius_downsample(p, 0.2, rank)[1].cpu().numpy()
    np.testing.assert_array_equal(a, b)
    for bb in (None, sc["bb"]):
        d1 = ops.nn_dist(p, t, 60.0, bb=bb).cpu().numpy()
        d2 = ops.nn_dist(p, t, 60.0, bb=bb).cpu().numpy()
        assert d1.tobytes() == d2.tobytes()


def _brute_gpu(q, t, maxdist):
    """fp64 brute force on the GPU with torch (separate elementwise ops: the same sums as the rule, no fused multiply-adds)."""
    q, t = q.double(), t.double()
    best = torch.full((q.shape[0],), float("inf"), dtype=torch.float64, device=q.device)
    for s in range(0, q.shape[0], 32):
        d = q[s:s + 32, None, :] - t[None]
        d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
        best[s:s + 32] = d2.min(dim=1).values
    b2 = float(maxdist) ** 2
    fragile = ((best - b2).abs() <= MR.REL * b2).cpu().numpy()
    return torch.where(best < b2, best.sqrt(), torch.full_like(best, float("inf"))).cpu().numpy(), fragile


@pytest.mark.parametrize("outliers_only", [False, True])
def test_scale_2m_queries_against_brute_force(env, outliers_only):
    L, ops, synthetic, M = env
    sc = synthetic.make_point_cloud_scene(2_000_000, 500_000, seed=11, outliers_only=outliers_only)
    p, t = _g(sc["pred"]), _g(sc["gt"])
    got = ops.nn_dist(p, t, 60.0).cpu().numpy()
    idx = np.random.default_rng(1).choice(p.shape[0], 10_000, replace=False)
    want, fragile = _brute_gpu(p[torch.from_numpy(idx).cuda()], t, 60.0)
    _agree(got[idx], want, fragile)
    if outliers_only:
        assert 0.6 < np.isfinite(want).mean() < 0.9 and want[np.isfinite(want)].min() > 29.0      # (z 30-70: beyond 60 is inf)
