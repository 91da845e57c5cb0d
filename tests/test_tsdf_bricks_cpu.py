"""CPU: the brick layout of the TSDF volume.  Why the brick mesh can be the dense mesh bit for bit -- the
allocation rule, checked with the numpy rules of tests/_tsdf_ref.py and tests/_tsdf_bricks_ref.py on the scene of the GPU tests --
and the host logic of the feature: the argument checks of the ops and of the C entry points, and run() of
evaluation/tsdf_fusion.py with ``tsdf_layout``."""
import ctypes as C
import functools
from argparse import Namespace

import numpy as np
import pytest
import torch

from tests import _tsdf_bricks_ref as BR
from tests import _tsdf_ref as TR
from wild_deep_mvs_amd import _lib as L, ops, synthetic
from wild_deep_mvs_amd.evaluation import tsdf_fusion as TF
from wild_deep_mvs_amd.utils import point_cloud as PC


@pytest.fixture(scope="module")
def scene():
    return BR.make_scene()


@pytest.fixture(scope="module")
def refs(scene):
    """{grid: (dense state, touched, allocation)}, computed once."""
    return {name: BR.reference(scene, name) for name in BR.GRIDS}


@pytest.fixture(scope="module")
def dense_mesh(refs):
    """{(grid, min_weight): TR.extract of the full dense state}."""
    cases = (("scene", 1), ("scene", 3), ("scene_thin", 1))
    return {(g, mw): TR.extract(refs[g][0], BR.GRIDS[g][1], BR.GRIDS[g][2], mw) for g, mw in cases}


def _same_mesh(a, b):
    return all(x.shape == y.shape and np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x,
                                                     y.view(np.uint32) if y.dtype == np.float32 else y) for x, y in zip(a, b))


@pytest.mark.parametrize("grid", list(BR.GRIDS))
def test_the_bit_rule_allocates_what_the_definition_does(refs, grid):
    st, touched, alloc = refs[grid]
    m = BR.masks(touched)
    assert np.array_equal(BR.allocate_from_masks(m), alloc)
    assert np.array_equal((m >> 13 & 1).astype(bool), BR.per_brick(touched))          # bit 13 = (0, 0, 0): the touched bricks
    got = ops.tsdf_bricks(torch.from_numpy(m), BR.GRIDS[grid][0])                     # the torch plumbing of the op is the same rule
    assert np.array_equal(got.directory.numpy(), BR.directory(alloc)) and np.array_equal(got.brick_ids.numpy(), BR.brick_ids(alloc))
    n = int(alloc.sum())
    assert got.tsdf_sum.shape == (n, 8, 8, 8) and got.rgb_sum.shape == (n, 8, 8, 8, 3) and got.weight.dtype == torch.int32
    assert all(int(a.abs().sum()) == 0 for a in got.arrays()) and got.views == 0
    if grid.startswith("scene"):
        assert 0 < n < alloc.size


@pytest.mark.parametrize("grid, min_weight", (("scene", 1), ("scene_thin", 1), ("scene", 3)))
def test_zeroing_the_bricks_that_are_not_allocated_leaves_the_mesh(refs, dense_mesh, grid, min_weight):
    st, touched, alloc = refs[grid]
    dims, origin, voxel, _ = BR.GRIDS[grid]
    want = dense_mesh[grid, min_weight]
    assert want[0].shape[0] > 1000 and want[2].shape[0] > 2000
    assert _same_mesh(TR.extract(BR.zeroed(st, alloc), origin, voxel, min_weight), want)
    # on this lattice at most half of the 504 bricks are allocated, and some observed voxels lie in the others
    assert alloc.size == 504 and 2 * int(alloc.sum()) <= alloc.size
    lost = (st["weight"] > 0) & (BR.zeroed(st, alloc)["weight"] == 0)
    print(f"{grid}: {int(BR.per_brick(touched).sum())} touched, {int(alloc.sum())} allocated bricks, {int(lost.sum())} observed voxels in the others")
    assert lost.any()


def test_the_touched_bricks_alone_lose_part_of_the_mesh(refs, dense_mesh):
    """At a truncation below a voxel a surface cell reaches into a brick that no touched point lies in: the neighbours are needed."""
    st, touched, alloc = refs["scene_thin"]
    dims, origin, voxel, _ = BR.GRIDS["scene_thin"]
    only = BR.per_brick(touched)
    assert only.sum() < alloc.sum() and not (only & ~alloc).any()
    assert not _same_mesh(TR.extract(BR.zeroed(st, only), origin, voxel, 1), dense_mesh["scene_thin", 1])


def test_scatter_and_gather_round_trip(refs):
    st, touched, alloc = refs["g35x29x11"]
    dims = BR.GRIDS["g35x29x11"][0]
    every = np.ones_like(alloc)
    pool = BR.gather(st, every)
    assert pool["rgb_sum"].shape == (every.sum(), 8, 8, 8, 3) and pool["weight"].shape == (every.sum(), 8, 8, 8)
    back = BR.scatter(pool, every, dims)
    assert all(np.array_equal(back[k], st[k]) and back[k].dtype == st[k].dtype for k in st)
    # x fastest inside a brick, bricks in ascending order: voxel (i, j, k) = (9, 2, 3) is local (1, 2, 3) of brick 1
    assert pool["weight"][1, 3, 2, 1] == st["weight"][3, 2, 9]
    assert (pool["weight"][-1, 11 - 8:] == 0).all()                                   # pool voxels beyond the lattice are zero
    part = BR.gather(st, alloc)
    assert all(np.array_equal(BR.gather(BR.scatter(part, alloc, dims), alloc)[k], part[k]) for k in part)


def test_extract_bricks_is_the_dense_mesh_reordered(refs, dense_mesh):
    st, touched, alloc = refs["scene"]
    dims, origin, voxel, _ = BR.GRIDS["scene"]
    xyz, rgb, faces, keys = BR.extract_bricks(st, alloc, origin, voxel, 1)
    dx, dr, df = dense_mesh["scene", 1]
    assert keys.dtype == np.int64 and len(np.unique(keys)) == len(keys) and not (np.diff(keys) > 0).all()
    order = np.argsort(keys)
    assert np.array_equal(xyz[order].view(np.uint32), dx.view(np.uint32)) and np.array_equal(rgb[order], dr)
    rank = np.empty(len(keys), dtype=np.int64)
    rank[order] = np.arange(len(keys))
    as_rows = lambda f: f[np.lexsort(f.T[::-1])]
    assert np.array_equal(as_rows(rank[faces]), as_rows(df.astype(np.int64)))
    assert (keys[faces[:, 0]] < keys[faces[:, 1]]).all() and (keys[faces[:, 0]] < keys[faces[:, 2]]).all()


def test_ops_check_their_arguments_on_cpu_tensors():
    depths = [torch.ones(5, 7)]
    cams = ops.geo_filter_cams(torch.eye(3)[None], torch.eye(3)[None], torch.zeros(1, 3, 1))
    good = dict(origin=(0.0, 0.0, 0.0), voxel=0.5, trunc=1.5)
    for bad, word in ((dict(origin=(0.0, 0.0)), "origin"), (dict(voxel=0.0), "voxel"), (dict(trunc=float("nan")), "trunc")):
        with pytest.raises(ValueError, match=f"pscv.tsdf_brick_probe: {word}"):
            ops.tsdf_brick_probe(depths, cams, (9, 8, 7), **dict(good, **bad))
    for dims in ((0, 2, 2), (2, 2), (2 ** 31, 2, 2), (2 ** 14 * 8, 2 ** 14 * 8, 64)):
        with pytest.raises(ValueError, match="pscv.tsdf_brick_probe: dims"):
            ops.tsdf_brick_probe(depths, cams, dims, **good)
    with pytest.raises(ValueError, match="depth map 0"):
        ops.tsdf_brick_probe([torch.ones(5, 7, dtype=torch.float64)], cams, (9, 8, 7), **good)
    with pytest.raises(ValueError, match="cams"):
        ops.tsdf_brick_probe(depths, cams[:, :29], (9, 8, 7), **good)
    with pytest.raises(ValueError, match="at least one"):
        ops.tsdf_brick_probe([], cams, (9, 8, 7), **good)
    with pytest.raises(RuntimeError, match="no CPU"):                       # valid arguments: there is no CPU path
        ops.tsdf_brick_probe(depths, cams, (2048, 2048, 1024), **good)      # (a lattice of 2^32 points is a valid one)
    masks = torch.zeros((1, 1, 2), dtype=torch.int32)
    masks[0, 0, 0] = 1 << 13 | 1 << 14                                       # brick 0 touched at its +x face
    with pytest.raises(ValueError, match="pscv.tsdf_bricks: masks"):
        ops.tsdf_bricks(masks.long(), (9, 8, 7))
    with pytest.raises(ValueError, match="pscv.tsdf_bricks: masks"):
        ops.tsdf_bricks(masks, (17, 8, 7))
    with pytest.raises(ValueError, match="max_bricks"):
        ops.tsdf_bricks(masks, (9, 8, 7), max_bricks=-1)
    with pytest.raises(ValueError, match=rf"2 bricks \({2 * 512 * 24} bytes of state\), more than max_bricks = 1"):
        ops.tsdf_bricks(masks, (9, 8, 7), max_bricks=1)
    br = ops.tsdf_bricks(masks, (9, 8, 7), max_bricks=2)
    assert br.directory.tolist() == [[[0, 1]]] and br.brick_ids.tolist() == [0, 1] and br.dims == (9, 8, 7)
    none = ops.tsdf_bricks(torch.zeros_like(masks), (9, 8, 7))
    assert none.brick_ids.shape == (0,) and none.tsdf_sum.shape == (0, 8, 8, 8) and (none.directory == -1).all()
    colors = [torch.zeros(5, 7, 3, dtype=torch.uint8)]
    with pytest.raises(ValueError, match="bricks must be"):
        ops.tsdf_brick_integrate(ops.tsdf_volume((9, 8, 7), "cpu"), depths, colors, cams, **good)
    with pytest.raises(ValueError, match="bricks.weight"):
        ops.tsdf_brick_integrate(ops.TsdfBricks(br.dims, br.directory, br.brick_ids, br.tsdf_sum, br.weight.long(), br.rgb_sum, br.cweight),
                                 depths, colors, cams, **good)
    with pytest.raises(ValueError, match="bricks.directory"):
        ops.tsdf_brick_integrate(ops.TsdfBricks((17, 8, 7), *[getattr(br, k) for k in ("directory", "brick_ids")], *br.arrays()),
                                 depths, colors, cams, **good)
    with pytest.raises(ValueError, match="as many colour"):
        ops.tsdf_brick_integrate(br, depths, [], cams, **good)
    with pytest.raises(ValueError, match="colours of view 0"):
        ops.tsdf_brick_integrate(br, depths, [torch.zeros(5, 6, 3, dtype=torch.uint8)], cams, **good)
    with pytest.raises(ValueError, match="pscv.tsdf_brick_integrate: trunc"):
        ops.tsdf_brick_integrate(br, depths, colors, cams, **dict(good, trunc=0.0))
    full = ops.TsdfBricks(br.dims, br.directory, br.brick_ids, *br.arrays(), views=ops.TSDF_MAX_VIEWS)
    with pytest.raises(ValueError, match="exceed the 65793"):
        ops.tsdf_brick_integrate(full, depths, colors, cams, **good)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.tsdf_brick_integrate(br, depths, colors, cams, **good)
    assert br.views == 0
    for bad, word in ((dict(min_weight=0), "min_weight"), (dict(min_weight=1.5), "min_weight"), (dict(voxel=-1.0), "voxel"),
                      (dict(origin="abc"), "origin")):
        with pytest.raises(ValueError, match=f"pscv.tsdf_brick_extract: {word}"):
            ops.tsdf_brick_extract(br, **dict(dict(origin=(0.0, 0.0, 0.0), voxel=0.5), **bad))
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.tsdf_brick_extract(br, origin=(0.0, 0.0, 0.0), voxel=0.5)


def test_exports_and_c_argument_checks():
    vp, i, l, d = C.c_void_p, C.c_int, C.c_long, C.c_double
    pp = C.POINTER(vp)
    assert L.PROTOTYPES["pscv_tsdf_brick_probe"] == (i, [pp, vp, i, vp, vp, vp, d, d, d, d, d, i, i, i, vp, vp])
    assert L.PROTOTYPES["pscv_tsdf_brick_integrate"] == (i, [pp, pp, vp, i, vp, vp, d, d, d, d, d, i, i, i, vp, i, vp, vp, vp, vp, vp])
    assert L.PROTOTYPES["pscv_tsdf_brick_mark"] == (i, [vp, vp, vp, vp, i, i, i, i, i, vp, vp])
    assert L.PROTOTYPES["pscv_tsdf_brick_emit_vertices"] == (i, [vp, vp, vp, vp, vp, vp, vp, vp, i, i, i, i, d, d, d, d, vp, vp, vp, l, vp])
    assert L.PROTOTYPES["pscv_tsdf_brick_emit_faces"] == (i, [vp, vp, vp, vp, vp, i, i, i, i, vp, l, vp])
    assert L.ABI_VERSION == 14
    lib = L.lib()
    one = (vp * 1)(64)                       # a non-null address; every call below is refused before it is used
    hw = (C.c_int * 2)(5, 7)
    nan, inf = float("nan"), float("inf")

    def refused(fn, ok, cases):
        for change, word in cases:
            args = list(ok)
            for k, v in change.items():
                args[k] = v
            assert fn(*args, None) == -1 and word in lib.pscv_last_error(), (word, lib.pscv_last_error())

    big = {11: 2 ** 14 * 8, 12: 2 ** 14 * 8, 13: 64}                         # 2^14 x 2^14 x 8 bricks = 2^31
    refused(lib.pscv_tsdf_brick_probe, [one, hw, 1, 64, 64, 64, 0.0, 0.0, 0.0, 0.5, 1.5, 9, 8, 7, 64],
            [({0: None}, b"null"), ({5: None}, b"null"), ({14: None}, b"null"), ({2: 0}, b"n_views"), ({2: 65}, b"n_views"),
             ({6: nan}, b"origin"), ({9: 0.0}, b"voxel"), ({10: inf}, b"trunc"), ({11: 0}, b"dims"), (big, b"bricks"),
             ({1: (C.c_int * 2)(5, 0)}, b"bad size"), ({0: (vp * 1)(None)}, b"view 0 has a null pointer")])
    ok = [one, one, hw, 1, 64, 64, 0.0, 0.0, 0.0, 0.5, 1.5, 9, 8, 7, 64, 2, 64, 64, 64, 64]
    refused(lib.pscv_tsdf_brick_integrate, ok,
            [({0: None}, b"null"), ({14: None}, b"null"), ({18: None}, b"null"), ({3: 65}, b"n_views"), ({8: inf}, b"origin"),
             ({9: nan}, b"voxel"), ({10: 0.0}, b"trunc"), ({12: -3}, b"dims"), (big, b"bricks"), ({15: -1}, b"n_bricks"),
             ({15: 2 ** 22}, b"n_bricks"), ({1: (vp * 1)(None)}, b"view 0 has a null pointer")])
    assert lib.pscv_tsdf_brick_integrate(*(ok[:14] + [None, 0, None, None, None, None]), None) == 0      # no bricks: nothing to launch
    refused(lib.pscv_tsdf_brick_mark, [64, 64, 64, 64, 2, 9, 8, 7, 1, 64],
            [({0: None}, b"null"), ({2: None}, b"null"), ({9: None}, b"null"), ({8: 0}, b"min_weight"), ({5: 0}, b"dims"),
             ({4: 2 ** 22}, b"n_bricks")])
    assert lib.pscv_tsdf_brick_mark(None, None, None, None, 0, 9, 8, 7, 1, None, None) == 0
    ev = [64, 64, 64, 64, 64, 64, 64, 64, 2, 9, 8, 7, 0.0, 0.0, 0.0, 0.5, 64, 64, None, 5]
    refused(lib.pscv_tsdf_brick_emit_vertices, ev,
            [({19: -1}, b"n_vertices"), ({19: 2 ** 31}, b"n_vertices"), ({15: 0.0}, b"voxel"), ({12: inf}, b"origin"), ({11: 0}, b"dims"),
             ({8: -1}, b"n_bricks"), ({6: None}, b"null"), ({16: None}, b"null")])
    assert lib.pscv_tsdf_brick_emit_vertices(*(ev[:16] + [None, None, None, 0]), None) == 0              # no vertices: nothing to launch
    ef = [64, 64, 64, 64, 64, 2, 9, 8, 7, 64, 5]
    refused(lib.pscv_tsdf_brick_emit_faces, ef,
            [({10: -1}, b"n_faces"), ({8: 0}, b"dims"), ({5: 2 ** 22}, b"n_bricks"), ({2: None}, b"null"), ({3: None}, b"null")])
    assert lib.pscv_tsdf_brick_emit_faces(None, None, None, None, None, 2, 9, 8, 7, None, 0, None) == 0


# ---- run() ------------------------------------------------------------------------------------------------------------------------
def _fake_ops(monkeypatch, seen):
    """The dense and the brick ops of evaluation/tsdf_fusion.py replaced by the numpy rules (states are dicts of numpy arrays)."""
    np_views = lambda depths, colors: ([d.numpy() for d in depths], [c.numpy() for c in colors])

    def fake_integrate(state, depths, colors, cams, *, origin, voxel, trunc):
        seen.update(layout="dense", dims=state["weight"].shape[::-1])
        TR.integrate(state, *np_views(depths, colors), cams.numpy(), origin, voxel, trunc)

    def fake_extract(state, *, origin, voxel, min_weight):
        return tuple(torch.from_numpy(a) for a in TR.extract(state, origin, voxel, min_weight))

    def fake_probe(depths, cams, dims, *, origin, voxel, trunc):
        blank = [np.zeros(d.shape + (3,), np.uint8) for d in depths]
        st = BR.integrate(dims, [d.numpy() for d in depths], blank, cams.numpy(), origin, voxel, trunc)
        return BR.masks(BR.touched(st))

    def fake_bricks(masks, dims, max_bricks=None):
        alloc = BR.allocate_from_masks(masks)
        seen.update(layout="bricks", dims=tuple(dims), bricks=int(alloc.sum()), of=alloc.size, max_bricks=max_bricks)
        return dict(alloc=alloc, dims=dims)

    def fake_brick_integrate(bricks, depths, colors, cams, *, origin, voxel, trunc):
        st = BR.integrate(bricks["dims"], *np_views(depths, colors), cams.numpy(), origin, voxel, trunc)
        bricks["state"] = BR.zeroed(st, bricks["alloc"])                        # what the pool holds: nothing of the other bricks

    def fake_brick_extract(bricks, *, origin, voxel, min_weight):
        return tuple(torch.from_numpy(a) for a in BR.extract_bricks(bricks["state"], bricks["alloc"], origin, voxel, min_weight)[:3])

    monkeypatch.setattr(TF.ops, "tsdf_volume", lambda dims, device: TR.volume(dims))
    for name, fn in (("tsdf_integrate", fake_integrate), ("tsdf_extract", fake_extract), ("tsdf_brick_probe", fake_probe),
                     ("tsdf_bricks", fake_bricks), ("tsdf_brick_integrate", fake_brick_integrate), ("tsdf_brick_extract", fake_brick_extract)):
        monkeypatch.setattr(TF.ops, name, fn)
    monkeypatch.setattr(TF, "fuse_tsdf_mesh", functools.partial(TF.fuse_tsdf_mesh, device="cpu"))


def _run_inputs(tmp_path, V=4, H=24, W=32, ds=2):
    sc = synthetic.make_fusion_scene(V, H, W, exact=True)
    args = Namespace(model="mvsnet", nviews=V, data_path=str(tmp_path), scene="scan1", downscale=ds, colmap=False, filter=False,
                     prob_threshold=0.5, override=True, tsdf_trunc_voxels=3, tsdf_min_weight=1)
    folder = f"{args.model}_{args.nviews}"
    dfold = tmp_path / "IntRes" / "depthmaps" / folder / "scan1"
    dfold.mkdir(parents=True)
    rng = np.random.default_rng(0)
    batches = []
    for v in range(V):
        name = f"{v:08d}"
        np.savez(dfold / f"{name}_out.npz", depthmap=sc["depths"][v].numpy(), probability=np.ones((H, W), np.float32))
        order = [v] + [u for u in range(V) if u != v]
        Kf = sc["K"].clone()
        Kf[:, :2] *= ds
        batches.append({"filename": [name], "imgs": torch.from_numpy(rng.random((1, V, 3, H * ds, W * ds), dtype=np.float32)),
                        "K": Kf.unsqueeze(0)[:, order], "R": sc["R"].unsqueeze(0)[:, order], "t": sc["t"].unsqueeze(0)[:, order]})
    return args, batches, tmp_path / "Meshes" / folder / f"{folder}scan1.ply"


def _rows(xyz, rgb, faces=None):
    """Vertex rows (xyz bits, rgb) as a sorted multiset, or the faces as a sorted multiset of their three vertex rows in stored order."""
    v = np.concatenate((np.ascontiguousarray(xyz).view(np.uint32).astype(np.int64), rgb.astype(np.int64)), axis=1)
    rows = v if faces is None else v[faces].reshape(len(faces), -1)
    return rows[np.lexsort(rows.T[::-1])]


def test_run_with_the_brick_layout_writes_the_dense_mesh(tmp_path, monkeypatch):
    seen = {}
    _fake_ops(monkeypatch, seen)
    args, batches, out = _run_inputs(tmp_path)
    assert TF.tsdf_options(Namespace(tsdf_layout="bricks", tsdf_max_bricks=7, tsdf_voxel=None)) == dict(layout="bricks", max_bricks=7)
    TF.run(batches, args)                                            # no tsdf_layout: the dense path, the bytes of before
    assert seen == dict(layout="dense", dims=(25, 21, 10))
    dense_bytes = out.read_bytes()
    dense = PC.read_mesh(out)
    args.tsdf_layout = None
    TF.run(batches, args)
    assert out.read_bytes() == dense_bytes
    args.tsdf_layout = "dense"
    TF.run(batches, args)
    assert out.read_bytes() == dense_bytes
    args.tsdf_layout, args.tsdf_max_bricks = "bricks", 20
    TF.run(batches, args)
    assert seen["layout"] == "bricks" and seen["dims"] == (25, 21, 10) and seen["of"] == 4 * 3 * 2 and seen["max_bricks"] == 20
    got = PC.read_mesh(out)
    assert len(got[0]) == len(dense[0]) > 500 and len(got[2]) == len(dense[2]) > 1000
    assert np.array_equal(_rows(got[0], got[1]), _rows(dense[0], dense[1]))
    assert np.array_equal(_rows(*got), _rows(*dense))
    with pytest.raises(ValueError, match="layout must be"):
        TF.fuse_tsdf_mesh([torch.ones(4, 5)], [torch.zeros(4, 5, 3, dtype=torch.uint8)], torch.eye(3)[None], torch.eye(3)[None],
                          torch.zeros(1, 3, 1), layout="hash")


def test_the_brick_layout_ignores_max_voxels(monkeypatch):
    seen = {}
    _fake_ops(monkeypatch, seen)
    sc = synthetic.make_fusion_scene(4, 24, 32, exact=True)
    with pytest.raises(ValueError, match="exceeds max_voxels"):
        TF.fuse_tsdf_mesh(sc["depths"], sc["colors"], sc["K"], sc["R"], sc["t"], max_voxels=5000)
    xyz, rgb, faces = TF.fuse_tsdf_mesh(sc["depths"], sc["colors"], sc["K"], sc["R"], sc["t"], max_voxels=5000, layout="bricks")
    assert seen["layout"] == "bricks" and xyz.shape[0] > 500
