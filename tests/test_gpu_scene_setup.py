"""GPU: scene set-up from a COLMAP sparse model (csrc/scene_setup.hip behind ops.sparse_pair_counts / ops.sparse_depth_ranges and
utils/colmap_utils.py).

The count matrices are integers built with integer atomics: they must EQUAL the numpy restatement's (tests/_scene_setup_ref.py)
on the reference-made fixture tests/golden/scene_tiny and on a synthetic scene of 70 images whose longest tracks exceed one wave.
``compute_src_imgs`` must return the reference's lists; ``compute_min_max_depth_yao`` its float64 ranges within 1e-6 relative:
the engine sorts float32 depths, one rounding of 6e-8 each, and a percentile interpolates two of them, so the bar leaves a
margin of about 16 roundings.  Also the smallest models at which the pair loop can go wrong, and the argument errors."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import _scene_setup_ref as SR

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from wild_deep_mvs_amd import _lib as L, ops
    from wild_deep_mvs_amd.utils import colmap_utils as CU
    L.lib()
    return L, ops, CU


@functools.lru_cache(maxsize=None)
def tiny():
    """(cameras, images, points, the reference's results, the restatement's results): read and computed once, never written to."""
    from wild_deep_mvs_amd.utils import colmap_model as CM
    d = os.path.join(GOLDEN, "scene_tiny")
    want = dict(np.load(os.path.join(GOLDEN, "scene_tiny.npz")))
    images, points = CM.read_images_binary(os.path.join(d, "images.bin")), CM.read_points3D_binary(os.path.join(d, "points3D.bin"))
    mine = SR.scene_setup(images, points, want["R"], want["t"], min_triangulation_angle=float(want["min_triangulation_angle"]),
                          nsrc=int(want["nsrc"]))
    return CM.read_cameras_binary(os.path.join(d, "cameras.bin")), images, points, want, mine


@functools.lru_cache(maxsize=None)
def scene70():
    sc = SR.scene_70()
    adj, tri, margin = SR.pair_counts(sc["xyz"], sc["track_off"], sc["track_img"], sc["R"], sc["t"], 5.0)
    lo, hi = SR.depth_ranges(sc["xyz"], sc["obs_img"], sc["obs_pt"], sc["R"], sc["t"])
    return sc, adj, tri, margin, lo, hi


def _counts(ops, xyz, off, img, R, t, angle=5.0):
    d = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).cuda()
    adj, tri = ops.sparse_pair_counts(d(xyz, torch.float64), d(off, torch.int64), d(img, torch.int32), d(R, torch.float32),
                                      d(np.asarray(t).reshape(-1, 3), torch.float32), angle)
    n = len(R)
    assert adj.dtype == tri.dtype == torch.int32 and adj.is_cuda and tuple(adj.shape) == tuple(tri.shape) == (n, n)
    return adj.cpu().numpy().astype(np.int64), tri.cpu().numpy().astype(np.int64)


def _same(got, want, name):
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{name}: {len(bad)} entries differ, first (i, j) = {bad[0].tolist()}: gpu {got[tuple(bad[0])]} restatement {want[tuple(bad[0])]}"


def test_pair_counts_equal_the_restatement_on_the_fixture(env):
    _, ops, _ = env
    _, images, points, want, mine = tiny()
    xyz, off, img, _, _ = SR.flatten_model(images, points)
    adj, tri = _counts(ops, xyz, off, img, want["R"], want["t"], float(want["min_triangulation_angle"]))
    _same(adj, mine["adj"], "adj")
    _same(tri, mine["adj_tri"], "adj_tri")
    assert np.diag(adj).sum() == len(img) and not np.diag(tri).any() and tri.sum() > 0


def test_pair_counts_equal_the_restatement_with_tracks_longer_than_a_wave(env):
    _, ops, _ = env
    sc, want_adj, want_tri, margin, _, _ = scene70()
    lengths = np.diff(sc["track_off"])
    assert lengths.max() == 70 and (lengths > 64).sum() >= 4 and (lengths == 64).any() and lengths.min() == 2 and len(lengths) == 2000
    print(f"70 images: {int((lengths ** 2).sum())} ordered pairs, smallest |angle - 5 degrees| = {margin:.3e}")
    # equality below holds only while no pair sits on the threshold: fp64 rounding (acos, contraction) moves an angle by ~1e-14 degrees
    assert margin > 1e-9, f"a pair lies {margin:.3e} degrees from the threshold: the scene cannot be compared for equality"
    adj, tri = _counts(ops, sc["xyz"], sc["track_off"], sc["track_img"], sc["R"], sc["t"])
    _same(adj, want_adj, "adj")
    _same(tri, want_tri, "adj_tri")
    again = _counts(ops, sc["xyz"], sc["track_off"], sc["track_img"], sc["R"], sc["t"])
    assert np.array_equal(again[0], adj) and np.array_equal(again[1], tri), "the outputs are zero-filled by every call"
    off = ~np.eye(70, dtype=bool)
    assert 0 < tri[off].sum() < adj[off].sum(), "some pairs pass the angle test, some fail"


def test_compute_src_imgs_returns_the_references_lists(env):
    _, _, CU = env
    _, images, points, want, _ = tiny()
    got = CU.compute_src_imgs(images, points, want["R"], want["t"], float(want["min_triangulation_angle"]), int(want["nsrc"]), None)
    assert isinstance(got, list) and all(isinstance(r, list) and all(isinstance(i, int) for i in r) for r in got)
    assert got == want["sel_idx"].tolist()
    assert CU.compute_src_imgs(images, points, torch.from_numpy(want["R"]), torch.from_numpy(want["t"]), 5.0, 4, None) == got


def test_depth_ranges_are_the_references_within_the_float32_rounding(env):
    _, _, CU = env
    _, images, points, want, _ = tiny()
    lo, hi, a, b = CU.compute_min_max_depth_yao(points, images, want["K"], want["R"], want["t"])
    assert a is None and b is None and lo.dtype == hi.dtype == np.float64 and lo.shape == hi.shape == (12,)
    empty = int(want["empty_image"])
    assert lo[empty] == 0 and hi[empty] == 0
    rel = np.maximum(np.abs(lo - want["depth_min"]) / np.maximum(want["depth_min"], 1e-30), np.abs(hi - want["depth_max"]) / np.maximum(want["depth_max"], 1e-30))
    rel[empty] = 0
    print(f"depth ranges: largest relative difference to the reference {rel.max():.3e}")
    assert rel.max() <= 1e-6 and (want["depth_min"][np.arange(12) != empty] > 0).all()
    with pytest.raises(ValueError, match="last rows"):
        CU.compute_min_max_depth_yao(points, images, want["K"] * 2, want["R"], want["t"])


def test_depth_ranges_on_segments_of_every_length(env):
    """70 images with several hundred observations each, other percentiles, and the observations in shuffled order."""
    _, ops, _ = env
    sc, _, _, _, want_lo, want_hi = scene70()
    d = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).cuda()
    perm = np.random.default_rng(0).permutation(len(sc["obs_img"]))
    args = (d(sc["xyz"], torch.float64), d(sc["obs_img"][perm], torch.int32), d(sc["obs_pt"][perm], torch.int32), d(sc["R"], torch.float32),
            d(sc["t"], torch.float32))
    lo, hi = ops.sparse_depth_ranges(*args)
    assert lo.dtype == torch.float64 and lo.is_cuda and tuple(lo.shape) == (70,)
    np.testing.assert_allclose(lo.cpu().numpy(), want_lo, rtol=1e-6, atol=0)
    np.testing.assert_allclose(hi.cpu().numpy(), want_hi, rtol=1e-6, atol=0)
    lo, hi = ops.sparse_depth_ranges(*args, perc=(0, 50))
    w_lo, w_hi = SR.depth_ranges(sc["xyz"], sc["obs_img"], sc["obs_pt"], sc["R"], sc["t"], (0, 50))
    np.testing.assert_allclose(lo.cpu().numpy(), w_lo, rtol=1e-6, atol=0)
    np.testing.assert_allclose(hi.cpu().numpy(), w_hi, rtol=1e-6, atol=0)


def test_the_smallest_models(env):
    _, ops, _ = env
    R = np.stack([np.eye(3), np.eye(3), np.eye(3)]).astype(np.float32)
    t = np.array([[0, 0, 0], [-1, 0, 0], [-0.01, 0, 0]], dtype=np.float32)           # centres 0, 1 and 0.01 along x
    x = np.array([[0.0, 0.0, 4.0]])
    # one point, two images a baseline of 1 apart: atan(1 / 4) = 14 degrees both ways
    adj, tri = _counts(ops, x, [0, 2], [0, 1], R[:2], t[:2])
    assert adj.tolist() == [[1, 1], [1, 1]] and tri.tolist() == [[0, 1], [1, 0]]
    # ... 0.01 apart: 0.14 degrees; and with the threshold below that
    adj, tri = _counts(ops, x, [0, 2], [0, 2], R, t)
    assert adj.tolist() == [[1, 0, 1], [0, 0, 0], [1, 0, 1]] and not tri.any()
    adj, tri = _counts(ops, x, [0, 2], [0, 2], R, t, angle=0.1)
    assert tri.tolist() == [[0, 0, 1], [0, 0, 0], [1, 0, 0]]
    # a track of a single image: the diagonal alone; a point without a track; no point at all
    adj, tri = _counts(ops, np.concatenate([x, x + 1]), [0, 1, 1], [1], R, t)
    assert adj.tolist() == [[0, 0, 0], [0, 1, 0], [0, 0, 0]] and not tri.any()
    adj, tri = _counts(ops, np.zeros((0, 3)), [0], np.zeros(0, np.int32), R, t)
    assert not adj.any() and not tri.any()
    # the point at the origin has no direction: NaN cosine, never counted
    adj, tri = _counts(ops, np.zeros((1, 3)), [0, 2], [0, 1], R, t)
    assert adj.tolist() == [[1, 1, 0], [1, 1, 0], [0, 0, 0]] and not tri.any()
    # depth ranges: one observation is both percentiles; depth = z + t_z + 1e-6
    d = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).cuda()
    lo, hi = ops.sparse_depth_ranges(d(x, torch.float64), d([1], torch.int32), d([0], torch.int32), d(R, torch.float32), d(t, torch.float32))
    assert lo.tolist() == hi.tolist() == [0.0, float(np.float32(4.0 + 1e-6)), 0.0]
    lo, hi = ops.sparse_depth_ranges(d(x, torch.float64), d([], torch.int32), d([], torch.int32), d(R, torch.float32), d(t, torch.float32))
    assert lo.tolist() == hi.tolist() == [0.0, 0.0, 0.0]


def test_argument_errors(env):
    L, ops, _ = env
    sc = scene70()[0]
    c = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt)
    cpu = (c(sc["xyz"], torch.float64), c(sc["track_off"], torch.int64), c(sc["track_img"], torch.int32), c(sc["R"], torch.float32),
           c(sc["t"], torch.float32))
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.sparse_pair_counts(*cpu, 5.0)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.sparse_depth_ranges(cpu[0], c(sc["obs_img"], torch.int32), c(sc["obs_pt"], torch.int32), cpu[3], cpu[4])
    xyz, off, img, R, t = (x.cuda() for x in cpu)
    with pytest.raises(ValueError, match="xyz fp64"):
        ops.sparse_pair_counts(xyz.float(), off, img, R, t, 5.0)
    with pytest.raises(ValueError, match="track_img"):
        ops.sparse_pair_counts(xyz, off, img.long(), R, t, 5.0)
    with pytest.raises(ValueError, match=r"outside \[0,70\)"):
        ops.sparse_pair_counts(xyz, off, img + 1, R, t, 5.0)
    with pytest.raises(ValueError, match="rise from 0"):
        ops.sparse_pair_counts(xyz, off + 1, img, R, t, 5.0)
    with pytest.raises(ValueError, match="P \\+ 1"):
        ops.sparse_pair_counts(xyz, off[:-1], img, R, t, 5.0)
    with pytest.raises(ValueError, match=">= 0"):
        ops.sparse_pair_counts(xyz, off, img, R, t, -1.0)
    with pytest.raises(ValueError, match="obs_pt"):
        ops.sparse_depth_ranges(xyz, img, img + 2000, R, t)
    lib = L.lib()
    assert lib.pscv_sparse_pair_counts(None, None, None, 0, 0, None, None, 3, 5.0, None, None, None) == -1
    assert b"null pointer" in lib.pscv_last_error()
    assert lib.pscv_segment_percentiles(None, 0, None, 0, 0.01, 0.99, None, None, None) == -1
    assert lib.pscv_sparse_obs_depths(None, 0, None, None, 5, None, None, 3, None, None) == -1
