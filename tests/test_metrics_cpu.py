"""CPU: the numpy rules of tests/_metrics_ref.py against the reference's own metrics (tests/golden/metrics_tiny.npz, written by
tests/golden/gen_golden_metrics.py), the PLY reader of utils/point_cloud.py, and the metrics module's imports."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _metrics_ref as MR
from wild_deep_mvs_amd.utils.point_cloud import read_ply, write_point_cloud

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(HERE, "golden", "metrics_tiny.npz")))


def _same(got, want, fragile):
    """inf / finite patterns and values equal except on fragile entries, which must be rare."""
    assert got.shape == want.shape and got.dtype == np.float64
    assert fragile.sum() <= max(2, fragile.size // 1000)
    ok = ~fragile
    np.testing.assert_array_equal(np.isinf(got[ok]), np.isinf(want[ok]))
    np.testing.assert_array_equal(got[ok], want[ok])


def test_mis_rule_matches_the_reference_reduce_pts(gold):
    nbrs, fragile = MR.neighbours(gold["pred"], float(gold["reduce_dst"]))
    assert not fragile
    rank = np.empty(len(nbrs), dtype=np.int64)
    rank[gold["reduce_perm"]] = np.arange(len(nbrs))
    seq = MR.greedy_mis(nbrs, gold["reduce_perm"])
    par, rounds = MR.mis_rounds(nbrs, rank)
    np.testing.assert_array_equal(seq, gold["reduce_mask"])
    np.testing.assert_array_equal(par, gold["reduce_mask"])
    assert 1 < rounds < 20 and 0 < gold["reduce_mask"].sum() < gold["reduce_mask"].size


def test_bounded_nn_rule_matches_chamfer_imw(gold):
    d, fragile = MR.nn_bounded(gold["small_from"], gold["small_to"], float(gold["imw_maxdist"]))
    _same(d, gold["imw_dist"], fragile)
    assert np.isinf(d).any() and np.isfinite(d).any()


def test_blocked_rule_matches_chamfer(gold):
    for src, dst, key in (("gt", "pred", "chamfer_gt_to_pred"), ("pred", "gt", "chamfer_pred_to_gt")):
        d, fragile = MR.chamfer_blocked(gold[src], gold[dst], gold["bb"], 60)
        _same(d, gold[key], fragile)
    d, _ = MR.chamfer_blocked(gold["pred"], gold["gt"], gold["bb"], 60)
    assert (d == 60).any() and np.isinf(d).any()


def test_golden_pickles_are_consistent_with_the_parts(gold):
    np.random.seed(int(gold["seed"]))
    perm = np.random.permutation(gold["pred"].shape[0])
    np.testing.assert_array_equal(perm, gold["reduce_perm"])
    kept = gold["pred"][gold["reduce_mask"]]
    d, fragile = MR.chamfer_blocked(kept, gold["gt"], gold["bb"], 60)
    _same(d, gold["dtu_dist_predToGt"], fragile)
    assert gold["dtu_abovePlane"].shape == (gold["gt"].shape[0], 1) and gold["dtu_abovePlane"].dtype == bool
    assert gold["dtu_validMask"].shape == (kept.shape[0],)


def test_read_ply_round_trips_write_point_cloud(tmp_path):
    rng = np.random.default_rng(3)
    xyz = rng.standard_normal((257, 3)).astype(np.float32)
    rgb = rng.integers(0, 256, (257, 3), dtype=np.uint8)
    path = tmp_path / "c.ply"
    write_point_cloud(path, xyz, rgb)
    data = read_ply(path)
    assert data.dtype.names == ("x", "y", "z", "red", "green", "blue")
    np.testing.assert_array_equal(np.stack((data["x"], data["y"], data["z"]), 1), xyz)
    np.testing.assert_array_equal(np.stack((data["red"], data["green"], data["blue"]), 1), rgb)


def test_read_ply_reads_the_fusion_golden():
    sys.path.insert(0, os.path.join(HERE, "golden"))
    try:
        from gen_golden_fusion import golden_arrays
    finally:
        sys.path.pop(0)
    xyz, rgb = golden_arrays()
    data = read_ply(os.path.join(HERE, "golden", "fusion_points.ply"))
    np.testing.assert_array_equal(np.stack((data["x"], data["y"], data["z"]), 1), xyz)
    np.testing.assert_array_equal(np.stack((data["red"], data["green"], data["blue"]), 1), rgb)


def test_read_ply_rejects_float64_coordinates(tmp_path):
    path = tmp_path / "wide.ply"
    head = "ply\nformat binary_little_endian 1.0\nelement vertex 2\nproperty float64 x\nproperty float64 y\nproperty float64 z\nend_header\n"
    with open(path, "wb") as fh:
        fh.write(head.encode())
        fh.write(np.zeros(6, dtype="<f8").tobytes())
    with pytest.raises(ValueError, match="wide.ply.*float64"):
        read_ply(path)


def test_read_ply_rejects_ascii(tmp_path):
    path = tmp_path / "a.ply"
    path.write_text("ply\nformat ascii 1.0\nelement vertex 0\nproperty float x\nend_header\n")
    with pytest.raises(ValueError, match="not binary"):
        read_ply(path)


def test_metrics_module_imports_without_scipy_or_h5py():
    code = ("import sys\n"
            "for m in ('scipy', 'scipy.io', 'scipy.spatial', 'h5py'): sys.modules[m] = None\n"
            "import wild_deep_mvs_amd.evaluation.metrics as M\n"
            "assert callable(M.run) and callable(M.load_gt)\n"
            "print('ok')\n")
    res = subprocess.run([sys.executable, "-c", code], cwd=REPO, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "ok" in res.stdout, res.stderr
