"""GPU: TSDF integration and marching-tetrahedra extraction (csrc/tsdf_fusion.hip, ops.tsdf_integrate / ops.tsdf_extract) against the
numpy float64 rules of tests/_tsdf_ref.py, and the evaluation/tsdf_fusion.py mirror end to end.

Both sides compute the same fp64 operations in the same order from the same fp32 / byte values (division is correctly rounded,
nothing is contracted), the kernel's culling may only skip what provably changes nothing and the reference culls nothing: every
state array, vertex, colour and face index must be equal bit for bit.  No tolerance anywhere."""
from argparse import Namespace

import numpy as np
import pytest
import torch

from tests import _tsdf_ref as TR

pytestmark = pytest.mark.gpu

# name: (dims, origin, voxel); trunc = 3 voxels.  The scene's plane lies near z = 4, its cameras in the plane z = 0 looking along +z
# (view 3 looks back along -z at a plane near z = -4).  "cull" reaches behind the cameras, far outside every frustum and
# beyond the deepest surface.
GRIDS = {
    "g1": ((1, 1, 1), (0.05, -0.02, 3.93), 0.2),
    "g2": ((2, 2, 2), (0.05, -0.02, 3.85), 0.2),
    "g33x9x5": ((33, 9, 5), (-3.21, -0.83, 3.62), 0.2),
    "g35x29x11": ((35, 29, 11), (-3.43, -2.81, 3.02), 0.2),
    "cull": ((70, 10, 18), (-25.03, -2.71, -2.04), 0.6),
}


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from wild_deep_mvs_amd import _lib as L, ops, synthetic
    L.lib()
    return L, ops, synthetic


@pytest.fixture(scope="module")
def scene(env):
    L, ops, synthetic = env
    sc = synthetic.make_fusion_scene(5, 24, 32, half_res_view=2, behind_view=3)
    depths = [d.clone() for d in sc["depths"]]
    depths[1][3, 4], depths[1][3, 5], depths[1][10, 20] = float("nan"), float("inf"), -2.5
    cams = ops.geo_filter_cams(sc["K"], sc["R"], sc["t"])
    return dict(depths=depths, colors=sc["colors"], cams=cams, sc=sc)


def _to_state(ops, st):
    nz, ny, nx = st["weight"].shape
    return ops.TsdfVolume((nx, ny, nz), *[torch.from_numpy(st[k].copy()).cuda() for k in ("tsdf_sum", "weight", "rgb_sum", "cweight")])


def _to_numpy(state):
    return dict(zip(("tsdf_sum", "weight", "rgb_sum", "cweight"), (a.cpu().numpy() for a in state.arrays())))


def _assert_state_equal(got, want):
    for k in ("weight", "cweight", "rgb_sum", "tsdf_sum"):
        a, b = got[k], want[k]
        assert a.dtype == b.dtype and a.shape == b.shape, k
        bits = np.uint32 if a.dtype == np.float32 else a.dtype
        diff = a.view(bits) != b.view(bits)
        assert not diff.any(), f"{k}: {int(diff.sum())} of {diff.size} entries differ, first at {np.argwhere(diff)[0]}"


@pytest.fixture(scope="module")
def integrated(env, scene):
    """{grid: (kernel state, reference state)} of the five views, shared by the integration and the extraction tests."""
    L, ops, synthetic = env
    out = {}
    for name, (dims, origin, voxel) in GRIDS.items():
        state = ops.tsdf_volume(dims)
        ops.tsdf_integrate(state, [d.cuda() for d in scene["depths"]], [c.cuda() for c in scene["colors"]], scene["cams"].cuda(),
                           origin=origin, voxel=voxel, trunc=3 * voxel)
        ref = TR.integrate(TR.volume(dims), [d.numpy() for d in scene["depths"]], [c.numpy() for c in scene["colors"]],
                           scene["cams"].numpy(), origin, voxel, 3 * voxel)
        out[name] = (state, ref)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("grid", list(GRIDS))
def test_integrate_equals_the_rule(integrated, grid):
    state, ref = integrated[grid]
    assert state.views == 5
    _assert_state_equal(_to_numpy(state), ref)
    if grid not in ("g1", "g2"):
        w = ref["weight"]
        assert w.max() >= 3 and (w == 0).any() and (ref["cweight"] < w).any() and (ref["cweight"] > 0).any()


def test_the_cull_grid_has_work_for_every_path(scene):
    """The grid named "cull" holds tiles wholly behind a camera, wholly left or right of, above and below a frustum and wholly too deep, next to
    tiles that are updated: decided here in float64 with the rule's own projection, with nothing of the kernel involved."""
    dims, origin, voxel = GRIDS["cull"]
    X, Y, Z = TR.lattice(dims, origin, voxel)
    cam = scene["cams"].numpy()[0]
    h, w = scene["depths"][0].shape
    x, y, z = TR.project(cam, X, Y, Z)
    first = lambda a: a[:, :4, :64].reshape(dims[2], -1)           # the first and the second 64 x 4 tile of every z plane
    second = lambda a: a[:, :4, 64:].reshape(dims[2], -1)
    with np.errstate(all="ignore"):
        outside = (x / z + 0.5 < -1.0) | (x / z + 0.5 > w + 1.0)
    assert (first(z) < -0.1).all(axis=1).any() and (second(outside) & (second(z) > 0)).all(axis=1).any()
    rows = lambda a, j0, j1: a[:, j0:j1, :64].reshape(dims[2], -1)   # the first x tile of the tile rows 0-3 and 8-9
    with np.errstate(all="ignore"):
        above, below = (y / z + 0.5 < -1.0) & (z > 0), (y / z + 0.5 > h + 1.0) & (z > 0)
    assert rows(above, 0, 4).all(axis=1).any() and rows(below, 8, 10).all(axis=1).any()
    d0 = scene["depths"][0].numpy()
    assert (first(z) > d0.max() + 3 * voxel + 0.5).all(axis=1).any()


def test_65_views_in_one_call_are_two_chunks(env, scene):
    L, ops, synthetic = env
    dims, origin, voxel = GRIDS["g33x9x5"]
    idx = [v % 5 for v in range(65)]
    depths, colors = [scene["depths"][v] for v in idx], [scene["colors"][v] for v in idx]
    cams = scene["cams"][idx]
    state = ops.tsdf_volume(dims)
    ops.tsdf_integrate(state, [d.cuda() for d in depths], [c.cuda() for c in colors], cams.cuda(), origin=origin, voxel=voxel,
                       trunc=3 * voxel)
    assert state.views == 65
    ref = TR.integrate(TR.volume(dims), [d.numpy() for d in depths], [c.numpy() for c in colors], cams.numpy(), origin, voxel, 3 * voxel)
    _assert_state_equal(_to_numpy(state), ref)
    assert ref["weight"].max() >= 39


def test_a_repeated_call_doubles_the_weights(env, scene, integrated):
    L, ops, synthetic = env
    dims, origin, voxel = GRIDS["g35x29x11"]
    first, ref = integrated["g35x29x11"]
    state = ops.TsdfVolume(first.dims, *[a.clone() for a in first.arrays()], views=first.views)
    packed = [ops.pack_rgba8(c.cuda()) for c in scene["colors"]]                  # the packed form of the colours is accepted too
    ops.tsdf_integrate(state, [d.cuda() for d in scene["depths"]], packed, scene["cams"].cuda(), origin=origin, voxel=voxel,
                       trunc=3 * voxel)
    twice = {k: v.copy() for k, v in ref.items()}
    TR.integrate(twice, [d.numpy() for d in scene["depths"]], [c.numpy() for c in scene["colors"]], scene["cams"].numpy(), origin,
                 voxel, 3 * voxel)
    got = _to_numpy(state)
    _assert_state_equal(got, twice)
    np.testing.assert_array_equal(got["weight"], 2 * ref["weight"])
    np.testing.assert_array_equal(got["cweight"], 2 * ref["cweight"])
    assert state.views == 10


# ---- extraction -------------------------------------------------------------------------------------------------------------------
def _sphere(n=14, radius=4.7, origin=(0.013, 0.027, 0.041)):
    st = TR.volume((n, n, n))
    X, Y, Z = TR.lattice((n, n, n), origin, 1.0)
    c = (n - 1) / 2.0
    st["tsdf_sum"][...] = (np.sqrt((X - c - origin[0]) ** 2 + (Y - c - origin[1]) ** 2 + (Z - c - origin[2]) ** 2) - radius).astype(np.float32)
    st["weight"][...] = 1
    return st


def _colours(st, rng):
    """Random colour sums: cweight 0..3 (0 on a third of the voxels), integer sums within 255 cweight."""
    cw = rng.integers(0, 4, st["cweight"].shape).astype(np.int32)
    st["cweight"][...] = cw
    st["rgb_sum"][...] = (rng.integers(0, 256, cw.shape + (3,)) * cw[..., None] - rng.integers(0, 2, cw.shape + (3,)) * (cw[..., None] > 0))
    st["rgb_sum"][...] = np.clip(st["rgb_sum"], 0, None)
    return st


def _hand_made(name):
    rng = np.random.default_rng(7)
    if name == "sphere":
        return _colours(_sphere(), rng)
    if name == "zero_plane":                                       # exact zeros on the lattice plane k = 3: zero counts as positive
        st = TR.volume((7, 6, 8))
        st["tsdf_sum"][...] = ((np.arange(8) - 3) * 0.5)[:, None, None]
        st["weight"][...] = 2
        return _colours(st, rng)
    if name == "alternating":                                      # the sign flips along every axis: every axis edge carries a vertex
        st = TR.volume((6, 5, 4))
        k, j, i = np.meshgrid(np.arange(4), np.arange(5), np.arange(6), indexing="ij")
        st["tsdf_sum"][...] = np.where((i + j + k) % 2 == 1, -1.0, 1.0) * (0.3 + 0.1 * ((3 * i + 5 * j + 7 * k) % 4))
        st["weight"][...] = 1 + (i + 2 * j) % 3
        return _colours(st, rng)
    if name == "random":                                           # random values, weights 0..3 and colours: every branch at once
        st = TR.volume((37, 7, 5))
        st["tsdf_sum"][...] = rng.standard_normal(st["tsdf_sum"].shape)
        st["weight"][...] = rng.integers(0, 4, st["weight"].shape)
        return _colours(st, rng)
    if name == "hole":
        st = _colours(_sphere(), rng)
        st["weight"][5:9, 4:8, 9:13] = 0
        return st
    if name == "unobserved":
        st = _colours(_sphere(), rng)
        st["weight"][...] = 0
        return st
    if name == "all_positive":
        st = _colours(_sphere(), rng)
        st["tsdf_sum"][...] = np.abs(st["tsdf_sum"])
        return st
    if name in ("flat_x", "flat_y", "flat_z"):                     # a 1 in one axis: edges and vertices, but no cell
        dims = {"flat_x": (1, 5, 6), "flat_y": (5, 1, 6), "flat_z": (5, 6, 1)}[name]
        st = TR.volume(dims)
        st["tsdf_sum"][...] = rng.standard_normal(st["tsdf_sum"].shape)
        st["weight"][...] = 1
        return _colours(st, rng)
    raise KeyError(name)


HAND_MADE = ("sphere", "zero_plane", "alternating", "random", "hole", "unobserved", "all_positive", "flat_x", "flat_y", "flat_z")
EMPTY = ("unobserved", "all_positive")


def _assert_mesh_equal(got, want):
    xyz, rgb, faces = (a.cpu().numpy() for a in got)
    assert xyz.dtype == np.float32 and rgb.dtype == np.uint8 and faces.dtype == np.int32
    assert xyz.shape == want[0].shape and faces.shape == want[2].shape, (xyz.shape, want[0].shape, faces.shape, want[2].shape)
    np.testing.assert_array_equal(xyz.view(np.uint32), want[0].view(np.uint32))
    np.testing.assert_array_equal(rgb, want[1])
    np.testing.assert_array_equal(faces, want[2])


@pytest.mark.parametrize("min_weight", (1, 3))
@pytest.mark.parametrize("name", HAND_MADE)
def test_extract_equals_the_rule_on_hand_made_volumes(env, name, min_weight):
    L, ops, synthetic = env
    st = _hand_made(name)
    origin, voxel = (0.013, 0.027, 0.041), (1.0 if "sphere" in name or name in ("hole",) + EMPTY else 0.37)
    want = TR.extract(st, origin, voxel, min_weight)
    got = ops.tsdf_extract(_to_state(ops, st), origin=origin, voxel=voxel, min_weight=min_weight)
    _assert_mesh_equal(got, want)
    nz, ny, nx = st["weight"].shape
    if name in EMPTY or (min_weight == 3 and name in ("sphere", "hole", "zero_plane", "flat_x", "flat_y", "flat_z")):
        assert want[0].shape[0] == 0 and want[2].shape[0] == 0
    elif name.startswith("flat"):
        assert want[0].shape[0] > 0 and want[2].shape[0] == 0
    elif name == "alternating" and min_weight == 3:                # isolated observed voxel pairs: vertices without a whole tetrahedron
        assert want[0].shape[0] > 0
    else:
        assert want[0].shape[0] > 0 and want[2].shape[0] > 0
    if name == "alternating" and min_weight == 1:
        assert want[0].shape[0] >= (nx - 1) * ny * nz + nx * (ny - 1) * nz + nx * ny * (nz - 1)


@pytest.mark.parametrize("min_weight", (1, 3))
@pytest.mark.parametrize("grid", ("g1", "g2", "g33x9x5", "g35x29x11", "cull"))
def test_extract_equals_the_rule_on_integrated_volumes(env, integrated, grid, min_weight):
    L, ops, synthetic = env
    dims, origin, voxel = GRIDS[grid]
    state, ref = integrated[grid]
    want = TR.extract(ref, origin, voxel, min_weight)
    _assert_mesh_equal(ops.tsdf_extract(state, origin=origin, voxel=voxel, min_weight=min_weight), want)
    if grid == "g35x29x11":
        assert want[0].shape[0] > 500 and want[2].shape[0] > 1000


# ---- end to end -------------------------------------------------------------------------------------------------------------------
def test_run_writes_the_mesh_and_the_metrics_read_its_points(env, tmp_path, monkeypatch, capsys):
    L, ops, synthetic = env
    from wild_deep_mvs_amd.evaluation import fusibile as EF, metrics as EM, tsdf_fusion as TF
    from wild_deep_mvs_amd.utils import point_cloud as PC
    V, H, W, ds = 5, 24, 32, 2
    sc = synthetic.make_fusion_scene(V, H, W, seed=5)
    args = Namespace(model="vis", nviews=V, data_path=str(tmp_path), scene="sceneA_3", downscale=ds, colmap=False, filter=False,
                     prob_threshold=0.5, override=False, tsdf_min_weight=2, tsdf_write_points=True, dataset="yfcc", override_fusion=True)
    folder = f"{args.model}_{args.nviews}"
    dfold = tmp_path / "IntRes" / "depthmaps" / folder / args.scene
    dfold.mkdir(parents=True)
    rng = np.random.default_rng(0)
    batches, masked, colors = [], [], []
    for v in range(V):
        name = f"{v:08d}"
        prob = np.ones((H, W), np.float32)
        if v == 0:
            prob[5:12, 8:20] = 0.2
        d = sc["depths"][v].numpy()
        np.savez(dfold / f"{name}_out.npz", depthmap=d, probability=prob)
        img = torch.from_numpy(rng.random((1, V, 3, H * ds, W * ds), dtype=np.float32))
        order = [v] + [u for u in range(V) if u != v]
        Kf = sc["K"].clone()
        Kf[:, :2] *= ds
        batches.append({"filename": [name], "imgs": img, "K": Kf.unsqueeze(0)[:, order], "R": sc["R"].unsqueeze(0)[:, order],
                        "t": sc["t"].unsqueeze(0)[:, order]})
        dm = d.copy()
        dm[prob < 0.5] = 0
        masked.append(dm)
        colors.append(EF.view_colors(img[0, 0], ds))
    TF.run(batches, args)
    out = tmp_path / "Meshes" / folder / f"{folder}{args.scene}.ply"
    xyz, rgb, faces = TF.fuse_tsdf_mesh(masked, colors, sc["K"], sc["R"], sc["t"], min_weight=2)
    assert xyz.shape[0] > 300 and faces.shape[0] > 500
    got = PC.read_mesh(out)
    np.testing.assert_array_equal(got[0], xyz.cpu().numpy())
    np.testing.assert_array_equal(got[1], rgb.cpu().numpy())
    np.testing.assert_array_equal(got[2], faces.cpu().numpy())
    # the vertices as a cloud: the metrics mirror runs on it
    monkeypatch.chdir(tmp_path)
    (tmp_path / "data" / "yfcc_subset_dataset" / "gt_resolution").mkdir(parents=True)
    (tmp_path / "data" / "yfcc_subset_dataset" / "gt_resolution" / "sceneA.txt").write_text("0.05\n")
    (tmp_path / "Points" / "gt").mkdir(parents=True)
    PC.write_point_cloud(tmp_path / "Points" / "gt" / "sceneA_gt.ply", got[0][::2], got[1][::2])
    EM.run(args)
    import pickle
    with open(tmp_path / "IntRes" / "chamfer" / folder / f"dists{args.scene}.pkl", "rb") as fh:
        res = pickle.load(fh)
    assert res["dist_predToGt"].shape == (xyz.shape[0],) and (res["dist_gtToPred"] == 0).all()
    # already computed: the file is left alone; override rewrites it
    stamp = out.read_bytes()
    out.write_bytes(b"stale")
    capsys.readouterr()
    TF.run(batches, args)
    assert "already computed" in capsys.readouterr().out and out.read_bytes() == b"stale"
    args.override = True
    TF.run(batches, args)
    assert out.read_bytes() == stamp
