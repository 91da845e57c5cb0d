"""CPU: the PatchMatch stereo rule of INTEGRATION.md section 2h as tests/_patch_match_ref.py states it, and the COLMAP ``Mat``
reader / writer of utils/colmap_array.py against files written by the reference's own ``write_array``."""
import math
import os

import numpy as np
import pytest
import torch

from tests import _patch_match_ref as PR
from wild_deep_mvs_amd import synthetic
from wild_deep_mvs_amd.utils.colmap_array import read_array, write_array

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "colmap_array")


def _gold_arrays():
    rng = np.random.default_rng(20261016)               # as tests/golden/gen_golden_colmap_array.py
    depth = rng.uniform(2.0, 8.0, (5, 7)).astype(np.float32)
    depth[1, 2] = 0.0
    return depth, rng.standard_normal((4, 6, 3)).astype(np.float32)


@pytest.mark.parametrize("name,idx", [("depth.bin", 0), ("normal.bin", 1)])
def test_mat_round_trip_matches_reference_writer(tmp_path, name, idx):
    want = _gold_arrays()[idx]
    got = read_array(os.path.join(GOLD, name))
    assert got.dtype == np.float32 and np.array_equal(got, want)
    write_array(got, tmp_path / name)
    assert (tmp_path / name).read_bytes() == open(os.path.join(GOLD, name), "rb").read()


def _lowbias32_py(x):
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def test_hash_known_values():
    assert [int(v) for v in PR.pm_hash(0, 0, [0, 1, 12345], 0, 0, 0)] == [1282570995, 1273722118, 3374369175]
    assert int(PR.pm_hash(7, 3, 999, 0xFFFFFFFF, 1, 5)) == 404744349
    assert int(PR.pm_hash(0xFFFFFFFF, 31, 2 ** 31 - 1, (1 << 16) | 7, 0, 2)) == 3593273806
    rng = np.random.default_rng(0)
    keys = rng.integers(0, 2 ** 32, (200, 6), dtype=np.uint64)
    for k in keys:
        h = _lowbias32_py(int(k[0]) ^ 0x9E3779B9)
        for word in k[1:]:
            h = _lowbias32_py(h ^ int(word))
        assert int(PR.pm_hash(*[int(x) for x in k])) == h
    u = PR.pm_uniform(1, 2, np.arange(100000), 3, 0, 4)
    assert u.min() >= 0.0 and u.max() < 1.0 and abs(u.mean() - 0.5) < 0.005
    assert np.array_equal(u * 2 ** 24, np.floor(u * 2 ** 24))          # 24-bit values: exact in fp32


def _two_view_cams(baseline=0.3, f=60.0, w=48, h=40, rot=0.05):
    K = np.array([[f, 0.0, w / 2.0], [0.0, f, h / 2.0], [0.0, 0.0, 1.0]])
    c, s = math.cos(rot), math.sin(rot)
    R1 = np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])
    Ks, Rs, ts = torch.tensor(np.stack([K, K])), torch.tensor(np.stack([np.eye(3), R1])), torch.tensor([[[0.0], [0.0], [0.0]],
                                                                                                      [[-baseline], [0.02], [0.01]]])
    from wild_deep_mvs_amd import ops
    return ops.geo_filter_cams(Ks, Rs, ts).numpy()


def test_homography_maps_plane_points_to_their_projection():
    cams = _two_view_cams()
    geo, Kinv = PR.source_geometry(cams)
    K1, R1, t1 = cams[1, 0:9].reshape(3, 3).astype(np.float64), cams[1, 18:27].reshape(3, 3).astype(np.float64), cams[1, 27:30].astype(np.float64)
    rng = np.random.default_rng(1)
    for _ in range(20):
        p = np.array([rng.uniform(0, 48), rng.uniform(0, 40), 1.0])
        d = rng.uniform(2.0, 6.0)
        n = rng.standard_normal(3)
        n /= np.linalg.norm(n)
        if n @ (Kinv @ p) > 0:
            n = -n
        X0 = d * Kinv @ p
        g = n @ Kinv / (n @ X0)
        H = geo[0]["A"] + np.outer(geo[0]["b"], g)
        # another pixel q: its ray meets the plane at X, whose true projection H q must be
        q = p + np.array([rng.uniform(-5, 5), rng.uniform(-5, 5), 0.0])
        m = Kinv @ q
        X = (n @ X0) / (n @ m) * m
        y = K1 @ (R1 @ X + t1)
        hq = H @ q
        assert np.allclose(hq[:2] / hq[2], y[:2] / y[2], atol=1e-9, rtol=0)


def test_fronto_parallel_plane_costs_zero_at_truth():
    """A textured plane z = Z seen by two cameras 4 px of disparity apart (pure x translation): at the true hypothesis every
    source sample lands on a pixel, so the NCC is 1 and c = 0; a wrong depth costs clearly more."""
    f, Z, w, h = 60.0, 3.0, 48, 40
    b = 4.0 * Z / f
    K = np.array([[f, 0.0, w / 2.0], [0.0, f, h / 2.0], [0.0, 0.0, 1.0]])
    from wild_deep_mvs_amd import ops
    cams = ops.geo_filter_cams(torch.tensor(np.stack([K, K])), torch.tensor(np.stack([np.eye(3)] * 2)),
                               torch.tensor([[[0.0], [0.0], [0.0]], [[-b], [0.0], [0.0]]])).numpy()
    ys, xs = np.meshgrid(np.arange(h), np.arange(w + 8), indexing="ij")
    X = (xs - w / 2.0) * Z / f
    Y = (ys - h / 2.0) * Z / f
    tex = (0.5 + 0.2 * np.sin(7.0 * X + 3.0 * Y) + 0.15 * np.cos(11.0 * Y - 5.0 * X ** 2)).astype(np.float32)
    ref = np.ascontiguousarray(tex[:, :w])
    src = np.ascontiguousarray(tex[:, 4:w + 4])                  # the source sees at x what the reference sees at x + 4
    rows, cols = np.divmod(np.arange(h * w), w)
    sel = (cols >= 10) & (cols < w - 6) & (rows >= 6) & (rows < h - 6)
    rows, cols = rows[sel], cols[sel]
    n = np.tile([0.0, 0.0, -1.0], (len(rows), 1))
    c, vr, _, _ = PR.source_costs(ref, [src], cams, rows, cols, np.full(len(rows), Z), n)
    assert (vr > PR.MIN_VAR).all()
    assert c.max() < 1e-9
    c_wrong, _, _, _ = PR.source_costs(ref, [src], cams, rows, cols, np.full(len(rows), Z * 1.2), n)
    assert np.median(c_wrong) > 0.01


def test_oracle_accuracy_on_tiny_scene():
    """The rule itself (numpy, fp64) on a 3-view 48 x 64 scene, which a CPU run finishes in about a minute.  The GPU test's kept
    bar holds here.  The other three are pinned at their measured levels with margins, because the scene is too small for the
    GPU bars: within 1 % 0.52 (1 % of depth is about 0.05 px of disparity), median normal error 10.2 deg, untextured filtered
    0.75 (the eroded disc has few pixels).  The GPU test checks the full bars at 96 x 128 and 192 x 256."""
    V, H, W = 3, 48, 64
    sc = synthetic.make_patch_match_scene(V, H, W, seed=0)
    greys = [PR.grey(sc["imgs"][v].numpy()) for v in range(V)]
    from wild_deep_mvs_amd import ops
    cams = ops.geo_filter_cams(sc["K"], sc["R"], sc["t"]).numpy()
    photo, geom, depth, normal = PR.reconstruct(greys, cams, sc["src"], sc["depth_min"].numpy(), sc["depth_max"].numpy())
    within, kept, nerr, untex = PR.accuracy(depth, normal, sc["depth"].numpy(), sc["normal"].numpy(), sc["untextured"].numpy(),
                                            sc["vis"].numpy())
    print(f"oracle {V} views {H}x{W}: within 1% {within:.3f}, kept {kept:.3f}, normal {nerr:.2f} deg, untextured out {untex:.3f}")
    assert within >= 0.45 and kept >= 0.70 and nerr <= 12.0 and untex >= 0.70
