"""GPU: the mesh metrics (csrc/mesh_metrics.hip behind ops.mesh_sample / ops.mesh_dist and the mesh functions of
evaluation/metrics.py) against the numpy rules of tests/_mesh_metrics_ref.py: samples and their faces
bit for bit, bounded distances to rtol 1e-12 with the inf pattern exact and the faces equal, the same bits for every cell size,
and the evaluation functions end to end.

Kernel and rules compute the same fp64 operations from the same float32 coordinates, so they agree everywhere; a disagreement of
a distance is tolerated only on `fragile` entries, whose squared distance lies within 1e-9 (relative) of the bound, and those
must be rare.  A sample count could differ only on a face whose A / spacing^2 + r lies within 1e-9 of an integer: the inputs have
none (asserted)."""
import pickle
from argparse import Namespace

import numpy as np
import pytest
import torch

from tests import _mesh_metrics_ref as R
from tests import _mesh_ref as MR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from wild_deep_mvs_amd import _lib as L, ops
    from wild_deep_mvs_amd.evaluation import metrics as M
    L.lib()
    return L, ops, M


def _g(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _agree(got, want, fragile=None, rtol=1e-12):
    """Same inf pattern, values to rtol; mismatches only on rare fragile entries (the pattern of tests/test_gpu_metrics.py)."""
    assert got.shape == want.shape and got.dtype == np.float64
    bad = (np.isinf(got) != np.isinf(want))
    fin = np.isfinite(got) & np.isfinite(want)
    bad |= fin & ~np.isclose(got, want, rtol=rtol, atol=0.0)
    if fragile is None:
        fragile = np.zeros(got.shape, dtype=bool)
    assert not (bad & ~fragile).any(), f"{int((bad & ~fragile).sum())} mismatches, e.g. {np.nonzero(bad & ~fragile)[0][:5]}"
    assert fragile.sum() <= max(2, got.size // 1000)


# ---------------------------------------------------------------------------------------------------------------------------
# sampling
def _sample_case(name):
    """(xyz, faces, spacing)"""
    if name == "one_triangle":
        return R.TRI_XYZ, R.TRI_FACES, 0.3
    if name == "zero_area":
        return np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0], [1, 0, 0]], dtype=np.float32), np.array([[0, 1, 3], [0, 1, 2]], dtype=np.int32), 0.3
    if name == "invalid_face":
        xyz = np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0], [1, 1, 3]], dtype=np.float32)
        return xyz, np.array([[0, 1, 2], [0, 1, 4], [-1, 2, 3], [1, 2, 3], [3, 3, 3]], dtype=np.int32), 0.25
    if name == "sphere":
        xyz, _, faces = MR.sphere_mesh()
        return xyz, faces, 0.5
    if name == "s14":                                       # 3977 faces: the scan crosses workgroups
        xyz, _, faces, _ = MR.scene_mesh("s14")
        return xyz, faces, 0.1
    if name == "big_triangle":                              # about 5000 samples: one face's samples cross workgroups
        return R.BIG_TRI_XYZ, R.TRI_FACES, float(np.sqrt(R.areas(R.BIG_TRI_XYZ, R.TRI_FACES)[0][0] / 5000.0))
    raise KeyError(name)


SAMPLE_CASES = ["one_triangle", "zero_area", "invalid_face", "sphere", "s14", "big_triangle"]


@pytest.mark.parametrize("name", SAMPLE_CASES)
def test_mesh_sample_equals_the_rule_bit_for_bit(env, name):
    L, ops, M = env
    xyz, faces, spacing = _sample_case(name)
    for seed in (0, 7):
        assert R.fragile_faces(xyz, faces, spacing, seed).size == 0
        want_pts, want_face = R.sample(xyz, faces, spacing, seed)
        pts, face = ops.mesh_sample(_g(xyz), _g(faces, np.int32), spacing, seed=seed, return_faces=True)
        assert pts.dtype == torch.float32 and face.dtype == torch.int32 and tuple(pts.shape) == (len(want_pts), 3)
        np.testing.assert_array_equal(face.cpu().numpy(), want_face)
        assert pts.cpu().numpy().tobytes() == want_pts.tobytes()
    assert len(want_pts) > 0
    if name == "s14":
        assert len(faces) == 3977
    if name == "big_triangle":
        assert abs(len(want_pts) - 5000) <= 1


def test_mesh_sample_is_deterministic_and_handles_empty_input(env):
    L, ops, M = env
    xyz, _, faces, _ = MR.scene_mesh("s14")
    gx, gf = _g(xyz), _g(faces, np.int32)
    a, fa = ops.mesh_sample(gx, gf, 0.1, seed=3, return_faces=True)
    b, fb = ops.mesh_sample(gx, gf, 0.1, seed=3, return_faces=True)
    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() and torch.equal(fa, fb)
    only = ops.mesh_sample(gx, gf, 0.1, seed=3)
    assert torch.is_tensor(only) and torch.equal(only, a)
    c = ops.mesh_sample(gx, gf, 0.1, seed=4)
    assert c.shape != a.shape or not torch.equal(c, a)
    # a 64-bit seed, negative or not, is taken modulo 2^64
    want = R.sample(xyz, faces, 0.1, 2 ** 64 - 5)[0]
    for seed in (2 ** 64 - 5, -5):
        assert ops.mesh_sample(gx, gf, 0.1, seed=seed).cpu().numpy().tobytes() == want.tobytes()
    pts, face = ops.mesh_sample(gx, gf[:0], 0.1, return_faces=True)
    assert tuple(pts.shape) == (0, 3) and tuple(face.shape) == (0,) and pts.dtype == torch.float32 and face.dtype == torch.int32
    pts = ops.mesh_sample(gx[:0], gf, 0.1)                  # no vertices: every face has an index out of range
    assert tuple(pts.shape) == (0, 3)
    with pytest.raises(ValueError, match="spacing 1e-06 gives"):
        ops.mesh_sample(gx, gf, 1e-6)


# ---------------------------------------------------------------------------------------------------------------------------
# distance
def _check_dist(ops, q, xyz, faces, maxdist, **kw):
    want, want_face, fragile = R.dist(q, xyz, faces, maxdist)
    got, face = ops.mesh_dist(_g(q), _g(xyz), _g(faces, np.int32), maxdist, return_faces=True, **kw)
    assert face.dtype == torch.int32
    got, face = got.cpu().numpy(), face.cpu().numpy()
    _agree(got, want, fragile)
    np.testing.assert_array_equal(face[~fragile], want_face[~fragile])
    assert ((face == -1) == np.isinf(got)).all()
    only = ops.mesh_dist(_g(q), _g(xyz), _g(faces, np.int32), maxdist, **kw)
    assert torch.is_tensor(only) and only.cpu().numpy().tobytes() == got.tobytes()
    return got, face


def test_mesh_dist_on_one_triangle_in_every_region(env):
    L, ops, M = env
    q = np.array([p for p, _ in R.REGIONS], dtype=np.float32)
    closed = np.array([d for _, d in R.REGIONS])
    got, face = _check_dist(ops, q, R.TRI_XYZ, R.TRI_FACES, 10.0)
    np.testing.assert_allclose(got, closed, rtol=1e-15, atol=0.0)
    assert (face == 0).all()
    got, face = _check_dist(ops, q, R.TRI_XYZ, R.TRI_FACES, 1.0)          # strict: the query at distance 1 is not below it
    assert np.isinf(got[closed >= 1.0]).all() and np.isfinite(got[closed < 1.0]).all()
    _check_dist(ops, q, R.TRI_XYZ, R.TRI_FACES, np.inf)


def test_mesh_dist_coincident_and_degenerate_faces(env):
    L, ops, M = env
    rng = np.random.default_rng(0)
    q = rng.uniform(-3, 3, (300, 3)).astype(np.float32)
    q[:len(R.REGIONS)] = [p for p, _ in R.REGIONS]
    # the same triangle three times behind another listing of it: the lowest index among equal d^2 wins
    faces = np.array([[0, 1, 2], [0, 1, 2], [0, 1, 2]], dtype=np.int32)
    got, face = _check_dist(ops, q, R.TRI_XYZ, faces, 100.0)
    assert (face == 0).all()
    got, face = _check_dist(ops, q, R.TRI_XYZ, np.array([[0, 1, 7], [0, 1, 2], [0, 1, 2]], dtype=np.int32), 100.0)
    assert (face == 1).all()
    # segments and a point
    got, face = _check_dist(ops, q, R.DEGENERATE_XYZ, R.DEGENERATE_FACES, 100.0)
    p = R.DEGENERATE_XYZ.astype(np.float64)
    seg = np.sqrt(R.segment_d2(q.astype(np.float64), p[0][None], p[1][None]))
    pnt = np.sqrt(((q.astype(np.float64) - p[3]) ** 2).sum(axis=1))
    np.testing.assert_allclose(got, np.minimum(seg, pnt), rtol=1e-12, atol=0.0)
    assert set(face.tolist()) <= {0, 1, 2, 3, 4} and (face[pnt < seg * (1 - 1e-9)] == 4).all()
    _check_dist(ops, q, R.DEGENERATE_XYZ, R.DEGENERATE_FACES, 1.5)


def test_mesh_dist_one_wide_triangle_over_many_cells(env):
    L, ops, M = env
    xyz = np.array([[0, 0, 0], [10, 0, 1], [0, 10, -1]], dtype=np.float32)
    rng = np.random.default_rng(2)
    q = rng.uniform([-3, -3, -3], [12, 12, 3], (1000, 3)).astype(np.float32)
    got, face = _check_dist(ops, q, xyz, R.TRI_FACES, 2.0, cell=0.5)
    assert 0.2 < np.isfinite(got).mean() < 0.9
    assert _check_dist(ops, q, xyz, R.TRI_FACES, 2.0)[0].tobytes() == got.tobytes()


@pytest.fixture(scope="module")
def s14_case():
    """(queries float32 [2000,3], xyz, faces, maxdist, h): 1000 within two voxels of the surface, 500 at mid range, 500 beyond."""
    xyz, _, faces, _ = MR.scene_mesh("s14")
    h, maxdist = 0.2, 1.0
    rng = np.random.default_rng(3)
    base = R.sample(xyz, faces, 0.05, seed=1)[0].astype(np.float64)
    base = base[rng.choice(len(base), 1500, replace=False)]
    unit = rng.normal(size=(1500, 3))
    unit /= np.linalg.norm(unit, axis=1, keepdims=True)
    near = base[:1000] + unit[:1000] * rng.uniform(0.0, 2 * h, (1000, 1))
    mid = base[1000:] + unit[1000:] * rng.uniform(2 * h, maxdist, (500, 1))
    lo, hi = xyz.min(axis=0), xyz.max(axis=0)
    far = rng.uniform(lo, hi, (500, 3))
    far[:, 2] = lo[2] - rng.uniform(1.2 * maxdist, 3.0 * maxdist, 500)          # below the whole mesh by more than maxdist
    q = np.concatenate((near, mid, far)).astype(np.float32)
    return q, xyz, faces, maxdist, h, R.dist(q, xyz, faces, maxdist)


def test_mesh_dist_on_the_scene_mesh_and_independence_of_the_index(env, s14_case):
    L, ops, M = env
    q, xyz, faces, maxdist, h, (want, want_face, fragile) = s14_case
    assert fragile.sum() <= 2 and np.isfinite(want[:1000]).all() and (want[:1000] <= 2 * h).all() and np.isinf(want[1500:]).all()
    assert np.isfinite(want[1000:1500]).all() and (want[1000:1500] > 2 * h).sum() > 50
    gq, gx, gf = _g(q), _g(xyz), _g(faces, np.int32)
    outs = []
    for cell in (None, h, 2 * h):
        d, face = ops.mesh_dist(gq, gx, gf, maxdist, return_faces=True, cell=cell)
        d, face = d.cpu().numpy(), face.cpu().numpy()
        _agree(d, want, fragile)
        np.testing.assert_array_equal(face[~fragile], want_face[~fragile])
        outs.append((d.tobytes(), face.tobytes()))
    assert outs[0] == outs[1] == outs[2]
    d2 = ops.mesh_dist(gq, gx, gf, maxdist)
    assert d2.cpu().numpy().tobytes() == outs[0][0]                             # two calls: the same bits


def test_mesh_dist_empty_inputs(env):
    L, ops, M = env
    xyz, _, faces = MR.sphere_mesh()
    q = _g(R.sphere_gt(50, 0))
    d, face = ops.mesh_dist(q, _g(xyz), _g(faces[:0], np.int32), 1.0, return_faces=True)
    assert d.dtype == torch.float64 and tuple(d.shape) == (50,) and bool(torch.isinf(d).all()) and bool((face == -1).all())
    bad = faces[:40].copy()
    bad[:, 1] = len(xyz)                                   # faces, but none of them valid: nothing is binned, every distance is inf
    bad[::2, 2] = -1
    d, face = ops.mesh_dist(q, _g(xyz), _g(bad, np.int32), 100.0, return_faces=True)
    assert bool(torch.isinf(d).all()) and bool((face == -1).all())
    d, face = ops.mesh_dist(q[:0], _g(xyz), _g(faces, np.int32), 1.0, return_faces=True)
    assert tuple(d.shape) == (0,) and tuple(face.shape) == (0,) and d.dtype == torch.float64 and face.dtype == torch.int32
    with pytest.raises(ValueError, match="finite"):
        ops.mesh_dist(torch.full((2, 3), float("nan"), device="cuda"), _g(xyz), _g(faces, np.int32), 1.0)
    with pytest.raises(ValueError, match="maxdist"):
        ops.mesh_dist(q, _g(xyz), _g(faces, np.int32), 0.0)
    # cells far smaller than the faces: the pair count (64-bit, every face saturated) exceeds 2^31 - 1 and the cell is named
    with pytest.raises(ValueError, match=r"^pscv.mesh_dist: cells of 1e-05 give \d+ \(cell, face\) pairs"):
        ops.mesh_dist(q, _g(xyz), _g(faces, np.int32), 1.0, cell=1e-5)


# ---------------------------------------------------------------------------------------------------------------------------
# evaluation
def test_mesh_to_cloud_dists_on_the_sphere(env):
    L, ops, M = env
    xyz, _, faces = MR.sphere_mesh()
    gt = R.sphere_gt(3000, 0)
    surf = M.mesh_to_cloud_dists(xyz, faces, gt, 2.0, spacing=0.25, seed=1)
    samp = M.mesh_to_cloud_dists(xyz, faces, gt, 2.0, spacing=0.25, seed=1, completeness="samples")
    pts, face = M.sample_mesh(xyz, faces, 0.25, seed=1)
    assert pts.dtype == np.float32 and face.dtype == np.int32 and len(pts) == len(face) > 3000
    assert surf["samples"].tobytes() == pts.tobytes() == samp["samples"].tobytes()
    # "samples": exactly today's functions on the sampled cloud
    assert samp["dist_gtToPred"].tobytes() == M.chamfer_imw(gt, pts, maxdist=2.0).tobytes()
    assert samp["dist_predToGt"].tobytes() == M.chamfer_imw(pts, gt, maxdist=2.0).tobytes() == surf["dist_predToGt"].tobytes()
    # "surface": the samples lie on the surface up to their rounding to float32, so the surface is never farther than they are
    eps = np.sqrt(3.0) * 2.0 ** -24 * float(np.abs(xyz).max())
    assert np.isfinite(surf["dist_gtToPred"]).all() and (surf["dist_gtToPred"] <= samp["dist_gtToPred"] + eps).all()
    _agree(surf["dist_gtToPred"][:300], R.dist(gt[:300], xyz, faces, 2.0)[0])
    # the level set of a unit grid lies within a fraction of a voxel of the analytic sphere
    assert surf["dist_gtToPred"].max() < 0.25


def test_run_mesh_dtu_end_to_end(env, tmp_path, monkeypatch):
    L, ops, M = env
    xyz, _, faces = MR.sphere_mesh()
    gt = R.sphere_gt(2000, 1)
    monkeypatch.setattr(M, "load_gt", lambda scene, path: R.dtu_gt(gt))
    R.write_mesh(tmp_path / "Meshes" / "mvsnet_3" / "mvsnet_3scan1.ply", xyz, faces)
    args = Namespace(dataset="dtu", model="mvsnet", nviews=3, scene="scan1", data_path=str(tmp_path), mesh_sample_seed=2)
    np.random.seed(4)
    M.run_mesh(args)
    out = tmp_path / "IntRes" / "chamfer_mesh" / "mvsnet_3" / "distsscan1.pkl"
    got = pickle.loads(out.read_bytes())
    assert set(got) == {"margin", "maxdist", "abovePlane", "validMask", "dist_gtToPred", "dist_predToGt"}
    assert got["margin"] == 10 and got["maxdist"] == 60
    np.random.seed(4)
    samples, _ = M.reduce_pts(M.sample_mesh(xyz, faces, 0.1, seed=2)[0], 0.2)   # the default spacing: half the 0.2 radius
    bb = R.dtu_gt(gt)[2]
    # kept samples lie more than 0.2 apart and leave no sample farther than 0.2 from all of them: area 278 over pi 0.2^2 .. pi 0.1^2
    assert 2000 < len(samples) < 9500
    assert got["validMask"].dtype == bool and got["validMask"].shape == (len(samples),)
    np.testing.assert_array_equal(got["validMask"], np.rint(samples[:, 0]) < 8)
    np.testing.assert_array_equal(got["abovePlane"][:, 0], gt[:, 2].astype(np.float64) - 6.5 > 0)
    assert got["dist_predToGt"].tobytes() == M.chamfer(samples, gt, bb, 60).tobytes()
    want, _, fragile = R.dist(gt[:400], xyz, faces, 60.0)
    _agree(got["dist_gtToPred"][:400], want, fragile)
    assert got["dist_gtToPred"].shape == (2000,) and np.isfinite(got["dist_gtToPred"]).all()
    before = out.read_bytes()
    M.run_mesh(args)                                                              # already computed: no work, no change
    assert out.read_bytes() == before
    args.override_fusion, args.mesh_completeness = True, "samples"
    np.random.seed(4)
    M.run_mesh(args)
    again = pickle.loads(out.read_bytes())
    assert again["dist_predToGt"].tobytes() == got["dist_predToGt"].tobytes()
    assert again["dist_gtToPred"].tobytes() == M.chamfer(gt, samples, bb, 60).tobytes()


def test_run_mesh_yfcc_end_to_end(env, tmp_path, monkeypatch):
    L, ops, M = env
    xyz, _, faces = MR.sphere_mesh()
    gt = R.sphere_gt(1500, 3)
    monkeypatch.chdir(tmp_path)
    (tmp_path / "data" / "yfcc_subset_dataset" / "gt_resolution").mkdir(parents=True)
    (tmp_path / "data" / "yfcc_subset_dataset" / "gt_resolution" / "sceneA.txt").write_text("0.25\n")
    R.write_cloud(tmp_path / "Points" / "gt" / "sceneA_gt.ply", gt)
    R.write_mesh(tmp_path / "Meshes" / "vis_5" / "vis_5sceneA_3.ply", xyz, faces)
    args = Namespace(dataset="yfcc", model="vis", nviews=5, scene="sceneA_3", data_path=str(tmp_path), override_fusion=True)
    M.run_mesh(args)
    got = pickle.loads((tmp_path / "IntRes" / "chamfer_mesh" / "vis_5" / "distssceneA_3.pkl").read_bytes())
    assert set(got) == {"dist_gtToPred", "dist_predToGt"}
    samples = R.sample(xyz, faces, 0.25, 0)[0]                                    # the default spacing: the scene's resolution
    assert got["dist_predToGt"].tobytes() == M.chamfer_imw(samples, gt, maxdist=2.5).tobytes()
    want, _, fragile = R.dist(gt[:400], xyz, faces, 2.5)
    _agree(got["dist_gtToPred"][:400], want, fragile)
    assert got["dist_gtToPred"].shape == (1500,)
