"""No GPU: the numpy rules of tests/_mesh_metrics_ref.py against hand-computed hashes, closed-form
distances and derived sampling bounds; the host checks of ops.mesh_sample / ops.mesh_dist; and the new functions of
evaluation/metrics.py with the operators replaced by the rules."""
import pickle
from argparse import Namespace

import numpy as np
import pytest
import torch

from tests import _mesh_metrics_ref as R
from tests import _mesh_ref as MR
from tests import _metrics_ref as PR
from wild_deep_mvs_amd import ops
from wild_deep_mvs_amd.evaluation import metrics as M

M64 = (1 << 64) - 1


# ---- hash -----------------------------------------------------------------------------------------------------------------------
def _mix(k):
    k ^= k >> 30
    k = k * 0xBF58476D1CE4E5B9 & M64
    k ^= k >> 27
    k = k * 0x94D049BB133111EB & M64
    return k ^ (k >> 31)


def _step(x):
    return _mix((x + 0x9E3779B97F4A7C15) & M64)


def test_hash_is_splitmix64():
    """step(x) is the output of splitmix64 after its state advanced from x: the published first outputs for the seeds 0 and
    1234567 (state + golden ratio, then the finaliser), and Python-integer arithmetic for the composed hashes."""
    g = 0x9E3779B97F4A7C15
    assert int(R.step(np.uint64(0))) == 0xE220A8397B1DCDAF
    assert int(R.step(np.uint64(g))) == 0x6E789E6AA1B965F4
    assert int(R.step(np.uint64(2 * g & M64))) == 0x06C45D188009454F
    assert int(R.step(np.uint64(1234567))) == 6457827717110365317
    assert int(R.step(np.uint64(1234567 + g))) == 3203168211198807973
    assert int(R.mix(np.uint64(0))) == 0
    for seed, f, k in ((0, 0, 0), (7, 5, 3), (2 ** 64 - 1, 3976, 4999), (-1, 1, 0)):
        hf = _step(_step(seed & M64) ^ f)
        assert int(R.face_hash(seed, f)) == hf
        assert int(R.sample_hash(np.uint64(hf), k)) == _step(hf ^ (k + 1))
    assert R.unit(np.uint64(M64)) == 1.0 - 2.0 ** -53 and R.unit(np.uint64(0)) == 0.0 and R.unit(np.uint64(1 << 63)) == 0.5
    r = R.unit(R.face_hash(3, np.arange(4096, dtype=np.uint64)))
    assert r.min() >= 0.0 and r.max() < 1.0 and abs(r.mean() - 0.5) < 6.0 / np.sqrt(12 * 4096)


# ---- distance -------------------------------------------------------------------------------------------------------------------
TRI_XYZ, TRI_FACES, REGIONS = R.TRI_XYZ, R.TRI_FACES, R.REGIONS


def test_dist_on_one_triangle_matches_closed_forms():
    q = np.array([p for p, _ in REGIONS], dtype=np.float32)
    want = np.array([d for _, d in REGIONS])
    d, face, fragile = R.dist(q, TRI_XYZ, TRI_FACES, 10.0)
    np.testing.assert_allclose(d, want, rtol=1e-15, atol=0.0)
    assert (face == 0).all() and not fragile.any()
    # the bound is strict, and the other orientation of the face gives the same distances
    d, face, fragile = R.dist(q, TRI_XYZ, TRI_FACES, 1.0)
    assert np.isinf(d[want >= 1.0]).all() and (face[want >= 1.0] == -1).all() and np.isfinite(d[want < 1.0]).all() and fragile[3]
    np.testing.assert_allclose(R.dist(q, TRI_XYZ, TRI_FACES[:, ::-1], 10.0)[0], want, rtol=1e-15, atol=0.0)


def test_degenerate_faces_are_segments_and_points():
    rng = np.random.default_rng(0)
    q = rng.uniform(-3, 3, (200, 3)).astype(np.float32)
    xyz = R.DEGENERATE_XYZ
    q64, p = q.astype(np.float64), xyz.astype(np.float64)
    seg = np.sqrt(R.segment_d2(q64, p[0][None], p[1][None]))
    for f in ([0, 1, 1], [0, 0, 1], [0, 2, 1], [1, 0, 2]):           # a repeated index, and three collinear corners
        d, face, _ = R.dist(q, xyz, np.array([f], dtype=np.int32), 100.0)
        np.testing.assert_allclose(d, seg, rtol=1e-12, atol=0.0)
    d, face, _ = R.dist(q, xyz, np.array([[3, 3, 3]], dtype=np.int32), 100.0)
    np.testing.assert_allclose(d, np.sqrt(((q64 - p[3]) ** 2).sum(axis=1)), rtol=1e-15, atol=0.0)
    # a face with an index out of range is skipped; coincident faces: the lowest index wins
    d, face, _ = R.dist(q, xyz, np.array([[0, 1, 4], [3, 3, 3], [3, 3, 3]], dtype=np.int32), 100.0)
    assert (face == 1).all()
    assert np.isinf(R.dist(q, xyz, np.array([[0, 1, -1]], dtype=np.int32), 100.0)[0]).all()


def _lattice(xyz, faces, n):
    """float64 [(n+1)(n+2)/2 * F, 3]: the corners of the n^2 congruent sub-triangles of every valid face."""
    p = np.asarray(xyz, dtype=np.float64)
    f = np.asarray(faces)[MR.valid_faces(faces, len(p))]
    a, b, c = p[f[:, 0]], p[f[:, 1]], p[f[:, 2]]
    return np.concatenate([a + (i / n) * (b - a) + (j / n) * (c - a) for i in range(n + 1) for j in range(n + 1 - i)])


def _min_point_dist(q, pts, chunk=64):
    q = np.asarray(q, dtype=np.float64)
    return np.concatenate([np.sqrt(((q[s:s + chunk, None, :] - pts[None]) ** 2).sum(axis=2).min(axis=1)) for s in range(0, len(q), chunk)])


@pytest.mark.parametrize("name", ["sphere", "s14"])
def test_dist_brackets_the_distance_to_dense_samples(name):
    """exact <= min over points of the surface <= exact + h.  Left: every such point is a point of the surface (the samples of
    `sample` up to their rounding to float32, at most sqrt(3) 2^-24 max|coordinate|; the lattice points up to float64 rounding,
    allowed as 1e-12).  Right, for the lattice of the n^2 congruent sub-triangles of every face: the nearest surface point lies in
    one sub-triangle, whose diameter is its longest edge, at most (the mesh's longest edge) / n = h, and whose corners are lattice
    points."""
    xyz, faces = (MR.sphere_mesh() if name == "sphere" else MR.scene_mesh("s14"))[0:3:2]
    rng = np.random.default_rng(1)
    lo, hi = xyz.min(axis=0), xyz.max(axis=0)
    q = rng.uniform(lo - 0.2 * (hi - lo), hi + 0.2 * (hi - lo), (120, 3)).astype(np.float32)
    exact, face, _ = R.dist(q, xyz, faces, np.inf)
    assert np.isfinite(exact).all() and (face >= 0).all()
    n = 4
    p = xyz.astype(np.float64)[faces[MR.valid_faces(faces, len(xyz))]]
    longest = np.sqrt(max(((p[:, i] - p[:, (i + 1) % 3]) ** 2).sum(axis=1).max() for i in range(3)))
    dense = _min_point_dist(q, _lattice(xyz, faces, n))
    assert (exact <= dense * (1 + 1e-12) + 1e-12).all()
    assert (dense <= exact + longest / n).all()
    spacing = 0.25 * np.sqrt(R.areas(xyz, faces)[0].mean())
    samples, _ = R.sample(xyz, faces, spacing, seed=5)
    assert len(samples) > 4 * len(faces)
    eps = np.sqrt(3.0) * 2.0 ** -24 * float(np.abs(xyz).max())
    assert (exact <= _min_point_dist(q, samples.astype(np.float64)) + eps).all()


# ---- sampling -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,spacing", [("sphere", 0.5), ("s14", 0.1)])
def test_sample_count_follows_the_area(name, spacing):
    """floor(x + U) has mean x and variance at most 1/4, so the total lies within 6 sigma = 3 sqrt(F) of area / spacing^2."""
    xyz, faces = (MR.sphere_mesh() if name == "sphere" else MR.scene_mesh("s14"))[0:3:2]
    A, good = R.areas(xyz, faces)
    for seed in (0, 1, 2):
        n = R.counts(xyz, faces, spacing, seed)
        assert (n[~good] == 0).all() and n.min() >= 0
        assert abs(int(n.sum()) - A[good].sum() / spacing ** 2) <= 3.0 * np.sqrt(len(faces))
        pts, face = R.sample(xyz, faces, spacing, seed)
        assert len(pts) == n.sum() and (np.bincount(face, minlength=len(faces)) == n).all() and (np.diff(face) >= 0).all()
    assert not np.array_equal(R.counts(xyz, faces, spacing, 0), R.counts(xyz, faces, spacing, 1))


def test_faces_without_samples():
    xyz = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 0], [np.nan, 0, 0], [np.inf, 1, 1]], dtype=np.float32)
    faces = np.array([[0, 1, 2], [0, 1, 3], [0, 1, 4], [0, 1, 6], [0, -1, 2], [0, 1, 5], [2, 2, 2], [1, 2, 0]], dtype=np.int32)
    n = R.counts(xyz, faces, 0.05, seed=4)
    assert (n[[1, 2, 3, 4, 5, 6]] == 0).all() and abs(n[0] - 200) <= 1 and abs(n[7] - 200) <= 1
    pts, face = R.sample(xyz, faces, 0.05, seed=4)
    assert set(face.tolist()) == {0, 7} and np.isfinite(pts).all()
    with pytest.raises(ValueError, match="spacing"):
        R.sample(xyz, faces, 1e-6)
    empty = R.sample(xyz, np.zeros((0, 3), dtype=np.int32), 0.1)
    assert empty[0].shape == (0, 3) and empty[1].shape == (0,)


@pytest.mark.parametrize("name,spacing", [("sphere", 0.5), ("s14", 0.1)])
def test_samples_lie_on_their_faces(name, spacing):
    xyz, faces = (MR.sphere_mesh() if name == "sphere" else MR.scene_mesh("s14"))[0:3:2]
    pts, face, uv = R.sample(xyz, faces, spacing, seed=2, return_uv=True)
    assert pts.dtype == np.float32 and face.dtype == np.int32
    w = 1.0 - uv[:, 0] - uv[:, 1]
    assert (uv >= 0.0).all() and (w >= -2.0 ** -52).all()                 # (1 - u - v: two roundings of numbers in [0, 1])
    p = xyz.astype(np.float64)
    a, b, c = p[faces[face, 0]], p[faces[face, 1]], p[faces[face, 2]]
    n = np.cross(b - a, c - a)
    off = np.abs(((pts.astype(np.float64) - a) * n).sum(axis=1)) / np.sqrt((n * n).sum(axis=1))
    # rounding each coordinate to float32 moves a point by at most 2^-24 |coordinate| per axis (the fp64 sum before it: 1e-12)
    assert (off <= np.sqrt(3.0) * 2.0 ** -24 * float(np.abs(xyz).max()) + 1e-12).all()


def test_samples_are_uniform_over_a_large_triangle():
    """About 5000 samples of one triangle, counted in its 16 congruent sub-triangles: Pearson's statistic against equal shares
    stays below the 0.999 quantile of chi-square with 15 degrees of freedom, 37.697 (three seeds; the draws are deterministic)."""
    xyz = R.BIG_TRI_XYZ
    A, _ = R.areas(xyz, TRI_FACES)
    spacing = float(np.sqrt(A[0] / 5000.0))
    for seed in (0, 1, 2):
        pts, face, uv = R.sample(xyz, TRI_FACES, spacing, seed, return_uv=True)
        assert abs(len(pts) - 5000) <= 1
        p = xyz.astype(np.float64)
        e = np.stack((p[1] - p[0], p[2] - p[0]), axis=1)                  # [3,2]
        st = np.linalg.lstsq(e, (pts.astype(np.float64) - p[0]).T, rcond=None)[0].T       # barycentric (u, v) of the float32 points
        assert np.abs(st - uv).max() < 1e-6
        s, t = np.clip(4.0 * st[:, 0], 0, 4 - 1e-9), np.clip(4.0 * st[:, 1], 0, 4 - 1e-9)
        i, j = np.floor(s).astype(int), np.floor(t).astype(int)
        upper = (s - i) + (t - j) > 1.0
        ok = i + j + upper <= 3
        cell = (i * 4 + j) * 2 + upper
        counts = np.unique(cell[ok], return_counts=True)
        assert len(counts[0]) == 16 and ok.sum() >= len(pts) - 2          # (a point on the long edge may round past it)
        expected = ok.sum() / 16.0
        assert ((counts[1] - expected) ** 2 / expected).sum() < 37.697


# ---- host checks of the operators -----------------------------------------------------------------------------------------------
def _mesh(device="cpu"):
    return torch.from_numpy(TRI_XYZ).to(device), torch.from_numpy(TRI_FACES).to(device)


def test_mesh_sample_names_one_bad_argument_without_a_gpu():
    xyz, faces = _mesh()
    cases = [("xyz", (xyz.double(), faces, 0.1), {}), ("xyz", (xyz[:, :2], faces, 0.1), {}), ("faces", (xyz, faces.long(), 0.1), {}),
             ("faces", (xyz, faces[:, :2], 0.1), {}), ("faces", (xyz, faces.reshape(-1), 0.1), {})]
    cases += [("spacing", (xyz, faces, s), {}) for s in (0.0, -1.0, float("nan"), float("inf"), 1e-200, 1e200, None, True)]
    cases += [("seed", (xyz, faces, 0.1), {"seed": s}) for s in (1.5, None, True)]
    cases += [("on the GPU", (xyz, faces, 0.1), {})]
    for phrase, args, kw in cases:
        with pytest.raises(ValueError, match=f"^pscv.mesh_sample: .*{phrase}"):
            ops.mesh_sample(*args, **kw)


def test_sample_and_pair_totals_that_overflow_are_named():
    assert ops._mesh_sample_total(2 ** 31 - 2, 0.001, "pscv.mesh_sample") == 2 ** 31 - 2
    with pytest.raises(ValueError, match=r"^pscv.mesh_sample: spacing 0.001 gives 2147483647 samples"):
        ops._mesh_sample_total(2 ** 31 - 1, 0.001, "pscv.mesh_sample")
    assert ops._mesh_pair_total(2 ** 31 - 1, 0.5, "pscv.mesh_dist") == 2 ** 31 - 1
    with pytest.raises(ValueError, match=r"^pscv.mesh_dist: cells of 0.5 give 2147483648 \(cell, face\) pairs"):
        ops._mesh_pair_total(2 ** 31, 0.5, "pscv.mesh_dist")
    assert ops._mesh_seed(-1, "x") == -1 and ops._mesh_seed(2 ** 64 - 1, "x") == -1 and ops._mesh_seed(2 ** 63, "x") == -2 ** 63
    # a spacing whose counts overflow: the rule saturates every face at 2^31 - 1 and the total names the spacing
    xyz = (TRI_XYZ * 1000.0).astype(np.float32)
    total = int(R.counts(np.concatenate((xyz, xyz)), np.array([[0, 1, 2], [3, 4, 5]], dtype=np.int32), 1e-3).sum())
    assert total == 2 * (2 ** 31 - 1)
    with pytest.raises(ValueError, match="spacing 0.001"):
        ops._mesh_sample_total(total, 1e-3, "pscv.mesh_sample")


def test_mesh_dist_names_one_bad_argument_without_a_gpu():
    xyz, faces = _mesh()
    q = torch.zeros(4, 3)
    bad_q, bad_xyz = q.clone(), xyz.clone()
    bad_q[2, 1] = float("nan")
    bad_xyz[0, 0] = float("inf")
    cases = [("query", (q.double(), xyz, faces, 1.0), {}), ("query", (q[:, :2], xyz, faces, 1.0), {}), ("query", (q[0], xyz, faces, 1.0), {}),
             ("xyz", (q, xyz.half(), faces, 1.0), {}), ("xyz", (q, xyz.reshape(-1), faces, 1.0), {}),
             ("faces", (q, xyz, faces.long(), 1.0), {}), ("faces", (q, xyz, faces[:, :2], 1.0), {}),
             ("query must be finite", (bad_q, xyz, faces, 1.0), {}), ("xyz must be finite", (q, bad_xyz, faces, 1.0), {})]
    cases += [("maxdist", (q, xyz, faces, md), {}) for md in (0.0, -1.0, float("nan"), None)]
    cases += [("cell", (q, xyz, faces, 1.0), {"cell": c}) for c in (0.0, -0.5, float("inf"), float("nan"), "x")]
    for phrase, args, kw in cases:
        with pytest.raises(ValueError, match=f"^pscv.mesh_dist: .*{phrase}"):
            ops.mesh_dist(*args, **kw)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.mesh_dist(q, xyz, faces, 1.0)


# ---- evaluation/metrics.py on a machine without a GPU: the operators replaced by the rules ---------------------------------------
@pytest.fixture
def rules(monkeypatch):
    """metrics.DEVICE = "cpu" and ops.mesh_sample / mesh_dist / nn_dist / radius_downsample computed by the numpy rules."""
    t = torch.from_numpy

    def mesh_sample(xyz, faces, spacing, *, seed=0, return_faces=False):
        pts, face = R.sample(xyz.numpy(), faces.numpy(), spacing, seed)
        return (t(pts), t(face)) if return_faces else t(pts)

    def mesh_dist(query, xyz, faces, maxdist, *, return_faces=False, cell=None):
        d, face, _ = R.dist(query.numpy(), xyz.numpy(), faces.numpy(), maxdist)
        return (t(d), t(face)) if return_faces else t(d)

    def nn_dist(query, target, maxdist, bb=None, *, fine_cell=None):
        q, g = query.numpy(), target.numpy()
        return t(PR.nn_bounded(q, g, maxdist)[0] if bb is None else PR.chamfer_blocked(q, g, bb, maxdist)[0])

    def radius_downsample(pts, dst, rank, *, check_every=4):
        mask = PR.greedy_mis(PR.neighbours(pts.numpy(), dst)[0], np.argsort(rank.numpy()))
        return pts[t(mask)], t(mask), 1

    monkeypatch.setattr(M, "DEVICE", "cpu")
    for name, fn in (("mesh_sample", mesh_sample), ("mesh_dist", mesh_dist), ("nn_dist", nn_dist), ("radius_downsample", radius_downsample)):
        monkeypatch.setattr(ops, name, fn)


_sphere_gt, _dtu_gt, _write_cloud, _write_mesh = R.sphere_gt, R.dtu_gt, R.write_cloud, R.write_mesh


def test_sample_mesh_and_both_completeness_modes(rules):
    xyz, _, faces = MR.sphere_mesh()
    gt = _sphere_gt(150, 0)
    pts, face = M.sample_mesh(xyz, faces, 1.0, seed=3)
    want = R.sample(xyz, faces, 1.0, 3)
    assert isinstance(pts, np.ndarray) and pts.tobytes() == want[0].tobytes() and face.tobytes() == want[1].tobytes()
    surf = M.mesh_to_cloud_dists(xyz, faces, gt, 2.0, spacing=1.0, seed=3)
    samp = M.mesh_to_cloud_dists(xyz, faces, gt, 2.0, spacing=1.0, seed=3, completeness="samples")
    assert set(surf) == set(samp) == {"samples", "dist_predToGt", "dist_gtToPred"}
    assert surf["samples"].tobytes() == pts.tobytes() and surf["dist_predToGt"].tobytes() == samp["dist_predToGt"].tobytes()
    # "samples" is what today's functions give on the sampled cloud; "surface" is the distance to the mesh itself
    assert samp["dist_gtToPred"].tobytes() == M.chamfer_imw(gt, pts, maxdist=2.0).tobytes()
    assert samp["dist_predToGt"].tobytes() == M.chamfer_imw(pts, gt, maxdist=2.0).tobytes()
    assert surf["dist_gtToPred"].tobytes() == R.dist(gt, xyz, faces, 2.0)[0].tobytes()
    eps = np.sqrt(3.0) * 2.0 ** -24 * float(np.abs(xyz).max())
    assert (surf["dist_gtToPred"] <= samp["dist_gtToPred"] + eps).all()
    with pytest.raises(ValueError, match="completeness"):
        M.mesh_to_cloud_dists(xyz, faces, gt, 2.0, spacing=1.0, completeness="vertices")
    with pytest.raises(ValueError, match="int32"):
        M.sample_mesh(xyz, faces.astype(np.int64), 1.0)


def test_run_mesh_dtu_paths_and_pickle_keys(rules, tmp_path, monkeypatch):
    xyz, _, faces = MR.sphere_mesh()
    gt = _sphere_gt(120, 1)
    monkeypatch.setattr(M, "load_gt", lambda scene, path: _dtu_gt(gt))
    _write_mesh(tmp_path / "Meshes" / "mvsnet_3" / "mvsnet_3scan1.ply", xyz, faces)
    args = Namespace(dataset="dtu", model="mvsnet", nviews=3, scene="scan1", data_path=str(tmp_path), mesh_sample_spacing=1.0,
                     mesh_sample_seed=2)
    np.random.seed(4)
    M.run_mesh(args)
    out = tmp_path / "IntRes" / "chamfer_mesh" / "mvsnet_3" / "distsscan1.pkl"
    got = pickle.loads(out.read_bytes())
    assert set(got) == {"margin", "maxdist", "abovePlane", "validMask", "dist_gtToPred", "dist_predToGt"}
    assert got["margin"] == 10 and got["maxdist"] == 60
    # the samples, thinned as eval_dtu thins its cloud (same seed, same draw)
    np.random.seed(4)
    samples, _ = M.reduce_pts(R.sample(xyz, faces, 1.0, 2)[0], 0.2)
    bb = _dtu_gt(gt)[2]
    assert got["validMask"].dtype == bool and got["validMask"].shape == (len(samples),)
    np.testing.assert_array_equal(got["validMask"], np.rint(samples[:, 0]) < 8)
    np.testing.assert_array_equal(got["abovePlane"][:, 0], gt[:, 2].astype(np.float64) - 6.5 > 0)
    assert got["dist_predToGt"].tobytes() == M.chamfer(samples, gt, bb, 60).tobytes()
    assert got["dist_gtToPred"].tobytes() == R.dist(gt, xyz, faces, 60.0)[0].tobytes()
    # already computed: nothing is read or written; override_fusion computes again, here in the "samples" mode
    before = out.read_bytes()
    monkeypatch.setattr(M, "eval_dtu_mesh", lambda *a: pytest.fail("computed again"))
    M.run_mesh(args)
    monkeypatch.undo()
    assert out.read_bytes() == before


def test_run_mesh_honours_override_and_the_samples_mode(rules, tmp_path, monkeypatch):
    xyz, _, faces = MR.sphere_mesh()
    gt = _sphere_gt(60, 2)
    monkeypatch.setattr(M, "load_gt", lambda scene, path: _dtu_gt(gt))
    _write_mesh(tmp_path / "Meshes" / "vis_5" / "vis_5scan9.ply", xyz, faces)
    args = Namespace(dataset="dtu", model="vis", nviews=5, scene="scan9", data_path=str(tmp_path), mesh_sample_spacing=1.5)
    out = tmp_path / "IntRes" / "chamfer_mesh" / "vis_5" / "distsscan9.pkl"
    np.random.seed(0)
    M.run_mesh(args)
    first = pickle.loads(out.read_bytes())
    args.mesh_completeness, args.override_fusion = "samples", True
    np.random.seed(0)
    M.run_mesh(args)
    second = pickle.loads(out.read_bytes())
    assert first["dist_predToGt"].tobytes() == second["dist_predToGt"].tobytes()
    np.random.seed(0)
    samples, _ = M.reduce_pts(R.sample(xyz, faces, 1.5, 0)[0], 0.2)
    assert second["dist_gtToPred"].tobytes() == M.chamfer(gt, samples, _dtu_gt(gt)[2], 60).tobytes()
    assert first["dist_gtToPred"].tobytes() != second["dist_gtToPred"].tobytes()


def test_run_mesh_yfcc_paths_and_pickle_keys(rules, tmp_path, monkeypatch):
    xyz, _, faces = MR.sphere_mesh()
    gt = _sphere_gt(100, 3)
    monkeypatch.chdir(tmp_path)
    (tmp_path / "data" / "yfcc_subset_dataset" / "gt_resolution").mkdir(parents=True)
    (tmp_path / "data" / "yfcc_subset_dataset" / "gt_resolution" / "sceneA.txt").write_text("0.75\n")
    _write_cloud(tmp_path / "Points" / "gt" / "sceneA_gt.ply", gt)
    _write_mesh(tmp_path / "Meshes" / "vis_5" / "vis_5sceneA_3.ply", xyz, faces)
    args = Namespace(dataset="yfcc", model="vis", nviews=5, scene="sceneA_3", data_path=str(tmp_path))
    M.run_mesh(args)
    got = pickle.loads((tmp_path / "IntRes" / "chamfer_mesh" / "vis_5" / "distssceneA_3.pkl").read_bytes())
    assert set(got) == {"dist_gtToPred", "dist_predToGt"}
    samples = R.sample(xyz, faces, 0.75, 0)[0]                            # the default spacing: the scene's resolution
    assert got["dist_predToGt"].tobytes() == PR.nn_bounded(samples, gt, 7.5)[0].tobytes()
    assert got["dist_gtToPred"].tobytes() == R.dist(gt, xyz, faces, 7.5)[0].tobytes()


def test_run_writes_the_same_bytes_with_the_new_arguments_present(rules, tmp_path, monkeypatch):
    gt, pred = _sphere_gt(150, 4), _sphere_gt(200, 5)
    monkeypatch.setattr(M, "load_gt", lambda scene, path: _dtu_gt(gt))
    blobs = []
    for k, extra in enumerate(({}, dict(mesh_sample_spacing=0.3, mesh_completeness="samples", mesh_sample_seed=9))):
        root = tmp_path / str(k)
        _write_cloud(root / "Points" / "mvsnet_3" / "mvsnet_3scan1.ply", pred)
        np.random.seed(1)
        M.run(Namespace(dataset="dtu", model="mvsnet", nviews=3, scene="scan1", data_path=str(root), **extra))
        assert not (root / "IntRes" / "chamfer_mesh").exists()
        blobs.append((root / "IntRes" / "chamfer" / "mvsnet_3" / "distsscan1.pkl").read_bytes())
    assert blobs[0] == blobs[1] and set(pickle.loads(blobs[0])) == {"margin", "maxdist", "abovePlane", "validMask", "dist_gtToPred",
                                                                    "dist_predToGt"}


# ---- the C entry points refuse the same limits (no call below gets far enough to touch the device) --------------------------------
A = 64                                                    # a non-null address that is never used


def _refused(name, *args):
    lib = ops.L.lib()
    assert getattr(lib, name)(*args) == -1, name
    return lib.pscv_last_error().decode()


def test_c_entry_points_refuse_bad_arguments():
    lib = ops.L.lib()
    big = 715827883                                       # 3 F = 2^31 + 1
    assert lib.pscv_mesh_scan_workspace(-1) == -1 and lib.pscv_mesh_scan_workspace(big) == -1 and lib.pscv_mesh_scan_workspace(0) == 256
    assert lib.pscv_mesh_scan_workspace(4097) == 16640 + 2 * 256 + 256     # the counts, two chunk sums and offsets of 8 bytes, a spare row
    assert lib.pscv_mesh_grid_workspace(-1) == -1 and lib.pscv_mesh_grid_workspace(2 ** 31) == -1 and lib.pscv_mesh_grid_workspace(0) > 0
    count = lambda **kw: [kw.get(k, v) for k, v in dict(xyz=A, faces=A, F=5, V=4, spacing=0.1, seed=0, off=A, total=A, ws=A, nbytes=1 << 20,
                                                      stream=None).items()]
    assert "n_faces=715827883" in _refused("pscv_mesh_sample_count", *count(F=big))
    assert "n_faces=-1" in _refused("pscv_mesh_sample_count", *count(F=-1))
    assert "n_vertices=2147483648" in _refused("pscv_mesh_sample_count", *count(V=2 ** 31))
    assert "null pointer" in _refused("pscv_mesh_sample_count", *count(faces=None))
    assert "null pointer" in _refused("pscv_mesh_sample_count", *count(total=None))
    for s in (0.0, -1.0, float("nan"), float("inf"), 1e-200, 1e200):
        assert "spacing" in _refused("pscv_mesh_sample_count", *count(spacing=s))
    assert "workspace of 8 bytes < 1024" in _refused("pscv_mesh_sample_count", *count(nbytes=8))
    emit = lambda **kw: [kw.get(k, v) for k, v in dict(xyz=A, faces=A, off=A, F=5, V=4, seed=0, N=7, out=A, face=None, stream=None).items()]
    assert "n_samples=2147483647" in _refused("pscv_mesh_sample_emit", *emit(N=2 ** 31 - 1))
    assert "n_samples=-1" in _refused("pscv_mesh_sample_emit", *emit(N=-1))
    assert "7 samples need faces" in _refused("pscv_mesh_sample_emit", *emit(F=0, faces=None))
    assert "7 samples need faces" in _refused("pscv_mesh_sample_emit", *emit(out=None))
    grid = lambda **kw: [kw.get(k, v) for k, v in dict(xyz=A, faces=A, F=5, V=4, ox=0.0, oy=0.0, oz=0.0, cell=0.5, off=A, total=A, ws=A,
                                                     nbytes=1 << 20, stream=None).items()]
    for c in (0.0, -1.0, float("nan"), float("inf")):
        assert "cell edge" in _refused("pscv_mesh_grid_count", *grid(cell=c))
    assert "origin finite" in _refused("pscv_mesh_grid_count", *grid(oy=float("nan")))
    assert "workspace of 8 bytes" in _refused("pscv_mesh_grid_count", *grid(nbytes=8))
    build = lambda **kw: [kw.get(k, v) for k, v in dict(xyz=A, faces=A, off=A, F=5, V=4, ox=0.0, oy=0.0, oz=0.0, cell=0.5, P=9, grid=A,
                                                      nbytes=1 << 30, stream=None).items()]
    assert "n_pairs=2147483648" in _refused("pscv_mesh_grid_build", *build(P=2 ** 31))
    assert "null pointer" in _refused("pscv_mesh_grid_build", *build(grid=None))
    assert f"grid buffer of 8 bytes < {lib.pscv_mesh_grid_workspace(9)}" in _refused("pscv_mesh_grid_build", *build(nbytes=8))
    dist = lambda **kw: [kw.get(k, v) for k, v in dict(q=A, m=3, xyz=A, faces=A, F=5, V=4, fine=A, fp=9, coarse=A, cp=9, ox=0.0, oy=0.0, oz=0.0,
                                                     fc=0.5, cc=1.0, fr=2, cr=5, maxdist=4.0, out=A, face=None, stream=None).items()]
    assert "null pointer" in _refused("pscv_mesh_point_dist", *dist(coarse=None))
    assert "null pointer" in _refused("pscv_mesh_point_dist", *dist(out=None))
    assert "bad sizes m=-1" in _refused("pscv_mesh_point_dist", *dist(m=-1))
    assert "cell edges" in _refused("pscv_mesh_point_dist", *dist(fc=0.0))
    assert "rings fine=9" in _refused("pscv_mesh_point_dist", *dist(fr=9))
    for md in (0.0, -1.0, float("nan"), float("inf")):
        assert "maxdist" in _refused("pscv_mesh_point_dist", *dist(maxdist=md))
    assert "5 coarse rings of 1 do not cover maxdist 4.5" in _refused("pscv_mesh_point_dist", *dist(maxdist=4.5))
