"""GPU: the brick layout of the TSDF volume (csrc/tsdf_bricks.hip, ops.tsdf_brick_*) against the numpy
rules of tests/_tsdf_ref.py and tests/_tsdf_bricks_ref.py, and against the dense layout through evaluation/tsdf_fusion.py.

The reference decides the allocation from the definition (touched points, their 26 neighbours, any per brick) and integrates and
extracts the DENSE volume, culling nothing; the brick side sees only its pool.  Every comparison is bit for bit: masks, directory,
pool state, vertices, colours, faces and keys, in order.  No tolerance anywhere.

The large lattice: 2048 x 2048 x 1024 points of 0.1 (2^32 points, 8.4 M directory bricks).  The scene sits near the lattice index
(1930, 1930, 930) -- a lattice of these dimensions has no index (8000, 8000, 4000) -- where lin exceeds 2^31 and every key with it."""
from argparse import Namespace

import numpy as np
import pytest
import torch

from tests import _tsdf_bricks_ref as BR
from tests import _tsdf_ref as TR
from tests.test_gpu_tsdf import EMPTY, HAND_MADE, _hand_made

pytestmark = pytest.mark.gpu

NAMES = ("tsdf_sum", "weight", "rgb_sum", "cweight")
BIG_DIMS, BIG_ORIGIN, BIG_VOXEL = (2048, 2048, 1024), (-193.83, -194.01, -90.18), 0.1
BIG_WINDOW, BIG_WINDOW_DIMS = (1896, 1904, 848), (80, 64, 120)      # holds every touched point with a brick to spare on every side


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from wild_deep_mvs_amd import _lib as L, ops, synthetic
    L.lib()
    return L, ops, synthetic


@pytest.fixture(scope="module")
def scene(env):
    sc = BR.make_scene()
    sc["gpu"] = ([d.cuda() for d in sc["depths"]], [c.cuda() for c in sc["colors"]], sc["cams"].cuda())
    return sc


@pytest.fixture(scope="module")
def refs(scene):
    """{grid: (dense state, touched, allocation)} from the numpy rules, computed once and left unchanged."""
    return {name: BR.reference(scene, name) for name in BR.GRIDS}


@pytest.fixture(scope="module")
def fused(env, scene, refs):
    """{grid: (masks, TsdfBricks)}: probe, allocate and integrate the five views on every grid."""
    L, ops, synthetic = env
    depths, colors, cams = scene["gpu"]
    out = {}
    for name, (dims, origin, voxel, tv) in BR.GRIDS.items():
        masks = ops.tsdf_brick_probe(depths, cams, dims, origin=origin, voxel=voxel, trunc=tv * voxel)
        bricks = ops.tsdf_bricks(masks, dims)
        ops.tsdf_brick_integrate(bricks, depths, colors, cams, origin=origin, voxel=voxel, trunc=tv * voxel)
        out[name] = (masks, bricks)
    torch.cuda.synchronize()
    return out


def _assert_bits_equal(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    bits = {np.dtype(np.float32): np.uint32}.get(got.dtype, got.dtype)
    diff = got.view(bits) != want.view(bits)
    assert not diff.any(), f"{what}: {int(diff.sum())} of {diff.size} entries differ, first at {np.argwhere(diff)[0]}"


def _assert_pool_equal(bricks, want):
    for k, a in zip(NAMES, bricks.arrays()):
        _assert_bits_equal(a.cpu().numpy(), want[k], k)


def _assert_mesh_equal(got, want):
    for a, b, what in zip(got, want, ("xyz", "rgb", "faces", "keys")):
        _assert_bits_equal(a.cpu().numpy(), b, what)
    assert len(got) == len(want) == 4


def _to_bricks(ops, st, alloc):
    """A dense numpy state scattered into a brick volume on the GPU with the bricks of ``alloc``."""
    nz, ny, nx = st["weight"].shape
    pool = BR.gather(st, alloc)
    return ops.TsdfBricks((nx, ny, nz), torch.from_numpy(BR.directory(alloc)).cuda(), torch.from_numpy(BR.brick_ids(alloc)).cuda(),
                          *[torch.from_numpy(pool[k]).cuda() for k in NAMES])


@pytest.mark.parametrize("grid", list(BR.GRIDS))
def test_masks_and_allocation_equal_the_definition(fused, refs, grid):
    st, touched, alloc = refs[grid]
    masks, bricks = fused[grid]
    _assert_bits_equal(masks.cpu().numpy(), BR.masks(touched), "masks")
    _assert_bits_equal(bricks.directory.cpu().numpy(), BR.directory(alloc), "directory")
    _assert_bits_equal(bricks.brick_ids.cpu().numpy(), BR.brick_ids(alloc), "brick_ids")
    if grid not in ("g1", "g2"):
        assert touched.any() and not touched.all()
    if grid in ("cull", "scene", "scene_thin"):
        assert not alloc.all()


@pytest.mark.parametrize("grid", list(BR.GRIDS))
def test_pool_state_equals_the_dense_rule_at_the_allocated_bricks(fused, refs, grid):
    st, touched, alloc = refs[grid]
    masks, bricks = fused[grid]
    assert bricks.views == 5
    _assert_pool_equal(bricks, BR.gather(st, alloc))
    dims = BR.GRIDS[grid][0]
    inside = BR.gather({"one": np.ones(dims[::-1], np.int32)}, alloc)["one"] == 1    # pool voxels outside the lattice are zero
    for a in bricks.arrays():
        assert not a.cpu().numpy()[~inside].any()
    if grid in ("g1", "g2", "g33x9x5"):                             # nz < 8: every brick reaches beyond the lattice
        assert not inside.all() or not alloc.any()
    if grid.startswith("scene"):
        assert ((st["weight"] > 0) & (BR.zeroed(st, alloc)["weight"] == 0)).any()   # free space the pool does not store


def test_65_views_are_two_chunks(env, scene):
    L, ops, synthetic = env
    dims, origin, voxel, tv = BR.GRIDS["g33x9x5"]
    idx = [v % 5 for v in range(65)]
    depths, colors, cams = [scene["depths"][v] for v in idx], [scene["colors"][v] for v in idx], scene["cams"][idx]
    st = BR.integrate(dims, [d.numpy() for d in depths], [c.numpy() for c in colors], cams.numpy(), origin, voxel, tv * voxel)
    alloc = BR.allocation(BR.touched(st))
    gd, gc, gcam = [d.cuda() for d in depths], [c.cuda() for c in colors], cams.cuda()
    masks = ops.tsdf_brick_probe(gd, gcam, dims, origin=origin, voxel=voxel, trunc=tv * voxel)
    _assert_bits_equal(masks.cpu().numpy(), BR.masks(BR.touched(st)), "masks")
    bricks = ops.tsdf_bricks(masks, dims)
    ops.tsdf_brick_integrate(bricks, gd, gc, gcam, origin=origin, voxel=voxel, trunc=tv * voxel)
    assert bricks.views == 65 and st["weight"].max() >= 39
    _assert_pool_equal(bricks, BR.gather(st, alloc))


@pytest.mark.parametrize("min_weight", (1, 3))
@pytest.mark.parametrize("grid", list(BR.GRIDS))
def test_extract_equals_the_dense_mesh_reordered_on_integrated_volumes(env, fused, refs, grid, min_weight):
    L, ops, synthetic = env
    dims, origin, voxel, tv = BR.GRIDS[grid]
    st, touched, alloc = refs[grid]
    want = BR.extract_bricks(st, alloc, origin, voxel, min_weight)
    got = ops.tsdf_brick_extract(fused[grid][1], origin=origin, voxel=voxel, min_weight=min_weight, return_keys=True)
    _assert_mesh_equal(got, want)
    assert len(ops.tsdf_brick_extract(fused[grid][1], origin=origin, voxel=voxel, min_weight=min_weight)) == 3
    if grid.startswith("scene"):
        assert want[0].shape[0] > 1000 and want[2].shape[0] > 2000
        assert not (np.diff(want[3]) > 0).all()                     # brick order is not key order: the rotation rule is exercised


@pytest.mark.parametrize("min_weight", (1, 3))
@pytest.mark.parametrize("name", HAND_MADE)
def test_extract_equals_the_dense_mesh_reordered_on_hand_made_volumes(env, name, min_weight):
    """The volumes of tests/test_gpu_tsdf.py (the 14^3 sphere crosses the brick border at 8), scattered into bricks once with every
    brick allocated and once with only the needed ones: a negative voxel counts as touched, its 26 neighbours as needed."""
    L, ops, synthetic = env
    st = _hand_made(name)
    origin, voxel = (0.013, 0.027, 0.041), (1.0 if "sphere" in name or name in ("hole",) + EMPTY else 0.37)
    with np.errstate(all="ignore"):
        negative = (st["weight"] > 0) & (st["tsdf_sum"].astype(np.float64) / st["weight"].astype(np.float64) < 0.0)
    needed = BR.allocation(negative)
    for alloc in (np.ones_like(needed), needed):
        want = BR.extract_bricks(st, alloc, origin, voxel, min_weight)
        got = ops.tsdf_brick_extract(_to_bricks(ops, st, alloc), origin=origin, voxel=voxel, min_weight=min_weight, return_keys=True)
        _assert_mesh_equal(got, want)
    if name in EMPTY:
        assert want[0].shape[0] == 0 and (name == "unobserved" or not needed.any())
    elif min_weight == 1:
        assert want[0].shape[0] > 0
    if name == "sphere" and min_weight == 1:
        assert needed.shape == (2, 2, 2) and want[2].shape[0] > 1000


def _rows(xyz, rgb, faces=None):
    """Vertex rows (xyz bits, rgb) as a sorted multiset, or the faces as a sorted multiset of their three vertex rows in stored order."""
    v = np.concatenate((np.ascontiguousarray(xyz).view(np.uint32).astype(np.int64), rgb.astype(np.int64)), axis=1)
    rows = v if faces is None else v[faces].reshape(len(faces), -1)
    return rows[np.lexsort(rows.T[::-1])]


@pytest.mark.parametrize("min_weight", (1, 2))
def test_fuse_tsdf_mesh_gives_the_dense_mesh_in_both_layouts(env, scene, min_weight):
    L, ops, synthetic = env
    from wild_deep_mvs_amd.evaluation import tsdf_fusion as TF
    sc = scene["sc"]
    mesh = {}
    for layout in ("dense", "bricks"):
        out = TF.fuse_tsdf_mesh(scene["depths"], scene["colors"], sc["K"], sc["R"], sc["t"], voxel=0.1, min_weight=min_weight, layout=layout)
        mesh[layout] = tuple(a.cpu().numpy() for a in out)
    dense, bricks = mesh["dense"], mesh["bricks"]
    assert len(dense[0]) > 1000 and len(dense[2]) > 2000
    assert np.array_equal(_rows(bricks[0], bricks[1]), _rows(dense[0], dense[1]))
    assert np.array_equal(_rows(*bricks), _rows(*dense))
    assert not np.array_equal(bricks[0].view(np.uint32), dense[0].view(np.uint32))    # (the order differs: the comparison is not vacuous)
    with pytest.raises(ValueError, match=r"bricks \(\d+ bytes of state\), more than max_bricks = 3"):
        TF.fuse_tsdf_mesh(scene["depths"], scene["colors"], sc["K"], sc["R"], sc["t"], voxel=0.1, layout="bricks", max_bricks=3)


def test_a_lattice_of_more_than_2_to_31_points(env, scene):
    """Masks, state and mesh equal the reference evaluated on the window that holds every allocated brick; lin and the keys exceed 2^31."""
    L, ops, synthetic = env
    depths, colors, cams = scene["gpu"]
    trunc = 3 * BIG_VOXEL
    assert BIG_DIMS[0] * BIG_DIMS[1] * BIG_DIMS[2] > 2 ** 31
    st = BR.integrate(BIG_WINDOW_DIMS, *scene["np"], BIG_ORIGIN, BIG_VOXEL, trunc, window=BIG_WINDOW)
    touched = BR.touched(st)
    k, j, i = np.nonzero(touched)
    for lo, hi, n in ((i.min(), i.max(), BIG_WINDOW_DIMS[0]), (j.min(), j.max(), BIG_WINDOW_DIMS[1]), (k.min(), k.max(), BIG_WINDOW_DIMS[2])):
        assert lo >= 8 and hi < n - 8                              # a brick to spare: the window's border allocates nothing
    alloc = BR.allocation(touched)
    wb = tuple(slice(w // 8, w // 8 + n // 8) for w, n in zip(BIG_WINDOW[::-1], BIG_WINDOW_DIMS[::-1]))
    masks = ops.tsdf_brick_probe(depths, cams, BIG_DIMS, origin=BIG_ORIGIN, voxel=BIG_VOXEL, trunc=trunc)
    assert masks.shape == (128, 256, 256)
    _assert_bits_equal(masks[wb].cpu().numpy(), BR.masks(touched), "masks")
    assert int((masks != 0).sum()) == int((masks[wb] != 0).sum())  # nothing outside the window
    bricks = ops.tsdf_bricks(masks, BIG_DIMS)
    _assert_bits_equal(bricks.directory[wb].cpu().numpy(), BR.directory(alloc), "directory")
    assert int((bricks.directory >= 0).sum()) == int(alloc.sum()) == bricks.brick_ids.shape[0]
    bz, by, bx = np.nonzero(alloc)
    ids = ((bz + BIG_WINDOW[2] // 8) * 256 + by + BIG_WINDOW[1] // 8) * 256 + bx + BIG_WINDOW[0] // 8
    _assert_bits_equal(bricks.brick_ids.cpu().numpy(), ids.astype(np.int32), "brick_ids")
    ops.tsdf_brick_integrate(bricks, depths, colors, cams, origin=BIG_ORIGIN, voxel=BIG_VOXEL, trunc=trunc)
    _assert_pool_equal(bricks, BR.gather(st, alloc))
    want = BR.extract_bricks(st, alloc, BIG_ORIGIN, BIG_VOXEL, 1, window=BIG_WINDOW, lattice_dims=BIG_DIMS)
    got = ops.tsdf_brick_extract(bricks, origin=BIG_ORIGIN, voxel=BIG_VOXEL, min_weight=1, return_keys=True)
    _assert_mesh_equal(got, want)
    assert want[0].shape[0] > 1000 and want[2].shape[0] > 2000 and want[3].min() > 7 * 2 ** 31


def test_run_with_the_brick_layout_end_to_end(env, tmp_path):
    L, ops, synthetic = env
    from wild_deep_mvs_amd.evaluation import fusibile as EF, tsdf_fusion as TF
    from wild_deep_mvs_amd.utils import point_cloud as PC
    V, H, W, ds = 5, 24, 32, 2
    sc = synthetic.make_fusion_scene(V, H, W, seed=5)
    args = Namespace(model="vis", nviews=V, data_path=str(tmp_path), scene="sceneA_3", downscale=ds, colmap=False, filter=False,
                     prob_threshold=0.5, override=False, tsdf_min_weight=2, tsdf_layout="bricks", tsdf_max_bricks=4096,
                     tsdf_vertex_normals=True)
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
    TF.run(batches, args)                                           # the brick mesh goes through clean_mesh and write_mesh as it is
    got = PC.read_mesh(tmp_path / "Meshes" / folder / f"{folder}{args.scene}.ply")
    mesh = TF.fuse_tsdf_mesh(masked, colors, sc["K"], sc["R"], sc["t"], min_weight=2, layout="bricks")
    xyz, rgb, faces, normals = TF.clean_mesh(*mesh, vertex_normals=True)
    assert xyz.shape[0] > 300 and faces.shape[0] > 500
    np.testing.assert_array_equal(got[0], xyz.cpu().numpy())
    np.testing.assert_array_equal(got[1], rgb.cpu().numpy())
    np.testing.assert_array_equal(got[2], faces.cpu().numpy())
    dense = tuple(a.cpu().numpy() for a in TF.fuse_tsdf_mesh(masked, colors, sc["K"], sc["R"], sc["t"], min_weight=2))
    raw = tuple(a.cpu().numpy() for a in mesh)
    assert np.array_equal(_rows(*raw), _rows(*dense))
