"""CPU: the depth-to-normal rule of tests/_depth_normals_ref.py against ground truth, the exactness
of its determinant, and the host logic of the feature (options of the two fusion mirrors, argument checks of ops.depth_normals,
the two exports).  The bars of the ground-truth test are those of the rule's numpy prototype: it measured at most 0.018 degrees on
plane pixels (bar 0.05: the margin covers fp32 K), 2.11 degrees on sphere pixels (bar 4) and 0.4 % fallbacks (bar 1 %: at most
12 of 3072 pixels, all on the sphere's silhouette).  The prototype's figures are those of min_support 6 (the default) at r = 2
and 4 and of min_support 3 at r = 1, which this file reproduces exactly (0.0179 deg, 2.102 deg, 12 pixels); at r = 1 the
default asks for 6 of 9 taps, so the four image corners (4 taps) and most of the silhouette fall back by design (57 pixels)."""
import ctypes as C
import itertools
from argparse import Namespace

import numpy as np
import pytest
import torch

from tests import _depth_normals_ref as DR
from wild_deep_mvs_amd import _lib as L, ops, synthetic

RADII = (1, 2, 4)
MIN_SUPPORT = {1: 3, 2: 6, 4: 6}


@pytest.fixture(scope="module")
def scene():
    sc = synthetic.make_patch_match_scene(4, 48, 64, seed=3)
    cams = ops.geo_filter_cams(sc["K"], sc["R"], sc["t"]).numpy()
    return sc, cams


def _all_in_window(mask, r):
    """True where the whole (2r+1)^2 window lies inside the image and inside ``mask``."""
    h, w = mask.shape
    out = np.zeros_like(mask)
    acc = np.ones((h - 2 * r, w - 2 * r), dtype=bool)
    for j, i in itertools.product(range(2 * r + 1), repeat=2):
        acc &= mask[j:j + h - 2 * r, i:i + w - 2 * r]
    out[r:h - r, r:w - r] = acc
    return out


@pytest.mark.parametrize("r", RADII)
def test_reference_recovers_the_true_normals(scene, r):
    sc, cams = scene
    for v in (0, 1):
        depth = sc["depth"][v].numpy()
        truth = sc["normal"][v].numpy().astype(np.float64)
        assert not ((depth > 3.8) & (depth < 4.1)).any()             # the sphere (about 2.7-3.5) and the plane (about 5) are apart
        sphere = depth < 4.0
        normal, support = DR.depth_normals(depth, cams[v], radius=r, min_support=MIN_SUPPORT[r])
        n = normal.astype(np.float64)
        ang = np.degrees(np.arccos(np.clip((n * truth).sum(-1), -1.0, 1.0)))
        full = support == (2 * r + 1) ** 2
        on_plane, on_sphere = full & _all_in_window(~sphere, r), full & _all_in_window(sphere, r)
        fallbacks = int((support < 0).sum())
        print(f"view {v} r={r}: plane {on_plane.sum()} px max {ang[on_plane].max():.4f} deg, sphere {on_sphere.sum()} px max "
              f"{ang[on_sphere].max():.3f} deg, fallbacks {fallbacks} of {depth.size}")
        assert on_plane.sum() > 1000 and on_sphere.sum() > 50
        assert ang[on_plane].max() <= 0.05
        assert ang[on_sphere].max() <= 4.0
        assert (support != 0).all() and fallbacks <= 0.01 * depth.size
        ys, xs = np.meshgrid(np.arange(48.0), np.arange(64.0), indexing="ij")
        ray = np.stack((xs, ys, np.ones_like(xs)), axis=-1) @ cams[v][DR.CAM_KINV:DR.CAM_KINV + 9].astype(np.float64).reshape(3, 3).T
        assert ((n * ray).sum(-1) < 0.0).all()                       # every normal faces the camera
        assert np.abs(np.linalg.norm(n, axis=-1) - 1.0).max() <= 1e-6


def _pattern_map(on, r, rng, off_kind):
    """A (2r+1)^2 depth map whose centre pixel counts exactly the taps of the boolean pattern ``on``."""
    d = np.where(on, 1.0 + 0.04 * rng.uniform(-1.0, 1.0, on.shape), 0.0).astype(np.float32)
    off = {"far": np.float32(2.0), "near": np.float32(0.5), "zero": np.float32(0.0), "nan": np.float32(np.nan),
           "inf": np.float32(np.inf), "negative": np.float32(-1.0)}[off_kind]
    d[~on] = off
    d[r, r] = 1.0
    return d


def _exact_det(on, r):
    pts = [(i - r, j - r) for j in range(2 * r + 1) for i in range(2 * r + 1) if on[j, i]]
    S = lambda f: sum(f(i, j) for i, j in pts)                       # Python integers
    m = [[S(lambda i, j: i * i), S(lambda i, j: i * j), S(lambda i, j: i)],
         [S(lambda i, j: i * j), S(lambda i, j: j * j), S(lambda i, j: j)],
         [S(lambda i, j: i), S(lambda i, j: j), len(pts)]]
    return (m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0])
            + m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]))


@pytest.mark.parametrize("r", RADII)
def test_det_is_the_exact_integer_determinant(r):
    rng = np.random.default_rng(r)
    cam = ops.geo_filter_cams(torch.tensor([[[50.0, 0.0, 4.2], [0.0, 51.0, 3.9], [0.0, 0.0, 1.0]]]), torch.eye(3)[None],
                              torch.zeros(1, 3, 1)).numpy()[0]
    s = 2 * r + 1
    kinds = ("far", "near", "zero", "nan", "inf", "negative")
    for trial in range(60):
        on = rng.random((s, s)) < rng.uniform(0.1, 0.9)
        on[r, r] = True
        d = _pattern_map(on, r, rng, kinds[trial % len(kinds)])
        normal, support, parts = DR.depth_normals(d, cam, radius=r, min_support=3, want_parts=True)
        assert int(parts["n"][r, r]) == int(on.sum())
        det = parts["det"][r, r]
        assert det == float(_exact_det(on, r)) and det >= 0.0
        if det == 0.0:
            assert support[r, r] == -int(on.sum())
    # collinear and single-tap patterns: det == 0 exactly, the fallback ray
    row, col, diag, single = (np.zeros((s, s), dtype=bool) for _ in range(4))
    row[r, :] = True
    col[:, r] = True
    diag[np.arange(s), np.arange(s)] = True
    single[r, r] = True
    Ki = cam[DR.CAM_KINV:DR.CAM_KINV + 9].astype(np.float64).reshape(3, 3)
    ray = -(Ki @ np.array([r, r, 1.0]))
    ray /= np.linalg.norm(ray)
    for on in (row, col, diag, single):
        d = _pattern_map(on, r, rng, "far")
        normal, support, parts = DR.depth_normals(d, cam, radius=r, min_support=3, want_parts=True)
        assert parts["det"][r, r] == 0.0 and _exact_det(on, r) == 0
        assert support[r, r] == -int(on.sum())
        np.testing.assert_allclose(normal[r, r], ray, atol=1e-7)


def test_invalid_pixels_get_zero(scene):
    sc, cams = scene
    d = sc["depth"][0].numpy().copy()
    d[3, 4], d[5, 6], d[7, 8], d[9, 10] = 0.0, np.nan, np.inf, -2.0
    normal, support = DR.depth_normals(d, cams[0])
    for y, x in ((3, 4), (5, 6), (7, 8), (9, 10)):
        assert support[y, x] == 0 and (normal[y, x] == 0.0).all()
    assert (support != 0).sum() == d.size - 4 and np.isfinite(normal).all()


# ---- host logic (fails without the feature) ---------------------------------------------------------------------------------------
class _Untouchable:
    def __iter__(self):
        raise AssertionError("the dataloader was read before the options were checked")


def test_fusion_normals_option_is_checked_before_any_file():
    from wild_deep_mvs_amd.evaluation import colmap_fusion as CF, fusibile as FU
    for run in (CF.colmap_fusion, FU.run):
        with pytest.raises(ValueError, match="fusion_normals"):
            run(_Untouchable(), Namespace(fusion_normals="bogus"))          # no data_path, no scene: nothing else was looked at
        with pytest.raises(ValueError, match="colmap"):
            run(_Untouchable(), Namespace(fusion_normals="depth", colmap=True))
    assert FU.normal_source(Namespace()) == "constant" and FU.normal_source(Namespace(fusion_normals="depth", colmap=False)) == "depth"
    assert FU.depth_normal_options(Namespace()) == {}
    assert FU.depth_normal_options(Namespace(fusion_normal_radius=3, fusion_normal_gate=0.1, fusion_normal_support=5)) == \
        dict(radius=3, rel_gate=0.1, min_support=5)


def test_ops_depth_normals_checks_its_arguments_on_cpu_tensors():
    depths = [torch.ones(5, 7)]
    cams = ops.geo_filter_cams(torch.eye(3)[None], torch.eye(3)[None], torch.zeros(1, 3, 1))
    for bad, word in ((dict(radius=0), "radius"), (dict(radius=5), "radius"), (dict(rel_gate=0.0), "rel_gate"),
                      (dict(rel_gate=-0.1), "rel_gate"), (dict(rel_gate=float("nan")), "rel_gate"),
                      (dict(rel_gate=float("inf")), "rel_gate"), (dict(min_support=2), "min_support"),
                      (dict(radius=1, min_support=10), "min_support")):
        with pytest.raises(ValueError, match=f"pscv.depth_normals: {word}"):
            ops.depth_normals(depths, cams, **bad)
    with pytest.raises(RuntimeError, match="no CPU"):                       # valid arguments: there is no CPU path
        ops.depth_normals(depths, cams)
    with pytest.raises(ValueError, match="1..64 normal maps"):
        ops.point_world_normals(torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), [], cams)
    with pytest.raises(ValueError, match="int32"):
        ops.point_world_normals(torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int32), [torch.zeros(5, 7, 3)], cams)


def test_exports_and_c_argument_checks():
    vp, i, l, d = C.c_void_p, C.c_int, C.c_long, C.c_double
    pp = C.POINTER(vp)
    assert L.PROTOTYPES["pscv_depth_normals"] == (i, [pp, vp, i, vp, i, d, i, pp, pp, vp])
    assert L.PROTOTYPES["pscv_point_world_normals"] == (i, [vp, vp, l, pp, vp, i, vp, vp, vp])
    assert L.ABI_VERSION == 14
    lib = L.lib()
    one = (vp * 1)(64)                       # a non-null address; every call below is refused before it is used
    hw = (C.c_int * 2)(5, 7)
    cases = [((None, hw, 1, 64, 2, 0.05, 6, one, None), b"null"), ((one, hw, 0, 64, 2, 0.05, 6, one, None), b"n_views"),
             ((one, hw, 65, 64, 2, 0.05, 6, one, None), b"n_views"), ((one, hw, 1, 64, 0, 0.05, 6, one, None), b"radius"),
             ((one, hw, 1, 64, 5, 0.05, 6, one, None), b"radius"), ((one, hw, 1, 64, 2, 0.0, 6, one, None), b"rel_gate"),
             ((one, hw, 1, 64, 2, float("inf"), 6, one, None), b"rel_gate"),
             ((one, hw, 1, 64, 2, float("nan"), 6, one, None), b"rel_gate"), ((one, hw, 1, 64, 2, 0.05, 2, one, None), b"min_support"),
             ((one, hw, 1, 64, 2, 0.05, 26, one, None), b"min_support"),
             ((one, (C.c_int * 2)(0, 7), 1, 64, 2, 0.05, 6, one, None), b"bad size"),
             ((one, hw, 1, 64, 2, 0.05, 6, (vp * 1)(None), None), b"view 0 has a null pointer")]
    for args, word in cases:
        assert lib.pscv_depth_normals(*args, None) == -1 and word in lib.pscv_last_error(), word
    assert lib.pscv_point_world_normals(None, None, -1, one, hw, 1, 64, None, None) == -1 and b"n_points" in lib.pscv_last_error()
    assert lib.pscv_point_world_normals(None, None, 0, one, hw, 65, 64, None, None) == -1 and b"n_views" in lib.pscv_last_error()
    assert lib.pscv_point_world_normals(None, None, 3, one, hw, 1, 64, None, None) == -1 and b"null" in lib.pscv_last_error()
    assert lib.pscv_point_world_normals(None, None, 0, one, hw, 1, 64, None, None) == 0          # no points: nothing to launch
