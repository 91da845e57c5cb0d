"""GPU: mesh clean-up (csrc/mesh_clean.hip; ops.mesh_components / mesh_vertex_normals / mesh_clean) against the numpy rules of
tests/_mesh_ref.py, and the clean-up step of the evaluation/tsdf_fusion.py mirror end to end.

The labels are the smallest vertex index of each component, the sizes are integer counts, the compaction keeps the order, and the
normals are the same fp64 operations in the same order from the same fp32 values (division and square root are correctly rounded,
nothing is contracted): everything must be equal bit for bit, whatever the schedule of the union-find.  No tolerance anywhere."""
from argparse import Namespace

import numpy as np
import pytest
import torch

from tests import _mesh_ref as MR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from wild_deep_mvs_amd import _lib as L, ops, synthetic
    L.lib()
    return L, ops, synthetic


def _hand_made(name):
    """(faces int32 [F,3], n_vertices)"""
    if name in ("s14", "s14_w3", "s11"):
        xyz, rgb, faces, _ = MR.scene_mesh(name)
        return faces, len(xyz)
    if name == "empty":
        return np.zeros((0, 3), np.int32), 0
    if name == "no_faces":
        return np.zeros((0, 3), np.int32), 5
    if name == "one_face":
        return np.array([[4, 1, 2]], np.int32), 6
    if name.startswith("disjoint"):
        f = int(name[8:])
        return MR.disjoint(f), 3 * f
    if name.startswith("strip_"):
        return MR.strip(4096, name[6:]), 4096
    if name == "two_fans":
        xyz, faces = MR.two_fans()
        return faces, len(xyz)
    if name == "repeated":
        return np.array([[3, 3, 5], [7, 8, 7], [9, 9, 9], [5, 7, 1]], np.int32), 11
    if name == "unused":                                           # vertices in no face at the start, in the middle and at the end
        return np.array([[2, 3, 4], [4, 5, 9], [10, 11, 12], [12, 10, 9]], np.int32), 16
    if name == "soup":
        return MR.soup()
    raise KeyError(name)


CASES = ("s14", "s14_w3", "s11", "empty", "no_faces", "one_face", "disjoint63", "disjoint64", "disjoint65", "disjoint257",
         "strip_ascending", "strip_descending", "strip_random", "two_fans", "repeated", "unused", "soup")
LARGE = ("strip_ascending", "strip_descending", "strip_random", "soup")


@pytest.fixture(scope="module")
def reference():
    """{case: (label, fcount, vcount)} by the numpy rules, computed once."""
    out = {}
    for name in CASES:
        faces, n = _hand_made(name)
        label = MR.components(faces, n)
        out[name] = (label,) + MR.sizes(label, faces)
    return out


@pytest.mark.parametrize("name", CASES)
def test_components_equal_the_rule(env, reference, name):
    L, ops, synthetic = env
    faces, n = _hand_made(name)
    want = reference[name]
    dev_faces = torch.from_numpy(faces).cuda()
    for _ in range(2 if name in LARGE else 1):                     # twice: both equal the rule, and so each other
        got = ops.mesh_components(dev_faces, n)
        for g, w, what in zip(got, want, ("label", "fcount", "vcount")):
            g = g.cpu().numpy()
            assert g.dtype == np.int32 and g.shape == (n,), what
            np.testing.assert_array_equal(g, w, err_msg=what)
    label, fcount, vcount = want
    if name == "two_fans":
        assert sorted(np.unique(label).tolist()) == [0, 7] and fcount[[0, 7]].tolist() == [6, 6] and vcount[[0, 7]].tolist() == [7, 7]
    if name == "unused":
        assert np.unique(label).tolist() == [0, 1, 2, 6, 7, 8, 13, 14, 15] and fcount[2] == 4 and vcount[2] == 8
    if name.startswith("strip"):
        assert (label == 0).all() and fcount[0] == 4094
    if name.startswith("disjoint"):
        assert (fcount > 0).sum() == len(faces) and fcount.max() == 1
    if name == "soup":
        assert 200 <= (fcount > 0).sum() <= 400 and len(faces) == 100_000


def test_faces_out_of_range_are_counted_and_join_nothing(env):
    L, ops, synthetic = env
    faces, n = MR.disjoint(40), 120
    faces = np.concatenate((faces, np.stack((faces[:-1, 0], faces[1:, 1], faces[1:, 2]), axis=1)))   # a chain through all of them
    faces[7, 1], faces[50, 2] = n, -1
    with pytest.raises(RuntimeError, match=r"pscv.mesh_components: 2 faces have an index outside"):
        ops.mesh_components(torch.from_numpy(faces).cuda(), n)
    status = torch.zeros(2, dtype=torch.int32, device="cuda")
    dev_faces = torch.from_numpy(faces).cuda()
    label, fcount, vcount = ops._mesh_components(dev_faces, len(faces), n, status)
    assert status.tolist() == [2, 0]
    want = MR.components(faces, n)                                  # the rule skips the two faces too
    np.testing.assert_array_equal(label.cpu().numpy(), want)
    np.testing.assert_array_equal(want, MR.components(np.delete(faces, [7, 50], axis=0), n))
    np.testing.assert_array_equal(fcount.cpu().numpy(), MR.sizes(want, faces)[0])
    assert int(fcount.sum()) == len(faces) - 2
    xyz = torch.from_numpy(np.random.default_rng(2).standard_normal((n, 3)).astype(np.float32)).cuda()
    with pytest.raises(RuntimeError, match=r"pscv.mesh_clean: 2 faces have an index outside"):
        ops.mesh_clean(xyz, torch.zeros(n, 3, dtype=torch.uint8, device="cuda"), dev_faces)
    with pytest.raises(RuntimeError, match=r"3 faces have an index outside"):
        ops.mesh_components(dev_faces[:3], 0)
    nrm = ops.mesh_vertex_normals(xyz, dev_faces)                   # a face out of range adds nothing
    np.testing.assert_array_equal(nrm.cpu().numpy().view(np.uint32), MR.vertex_normals(xyz.cpu().numpy(), faces).view(np.uint32))


def _normal_cases(name):
    if name in ("s14", "s14_w3", "s11"):
        return MR.scene_mesh(name)[0], MR.scene_mesh(name)[2]
    if name == "sphere":
        return MR.sphere_mesh()[0], MR.sphere_mesh()[2]
    if name == "zero_plane":
        return MR.zero_plane_mesh()[0], MR.zero_plane_mesh()[2]
    if name == "strip":
        return MR.strip_xyz(4096), MR.strip(4096, "random")
    if name == "odd":                                              # a zero-area face, a repeated index, a vertex in no face, huge values
        xyz = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [5, 5, 5], [2, 0, 0], [0, 0, 1], [3e30, 0, 0], [0, 3e30, 0], [1e-30, 2e-30, 0]],
                       dtype=np.float32)
        return xyz, np.array([[0, 1, 2], [0, 1, 4], [0, 0, 5], [1, 2, 5], [6, 7, 8], [6, 8, 7], [6, 7, 5]], dtype=np.int32)
    if name == "empty":
        return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
    if name == "no_faces":
        return np.ones((5, 3), np.float32), np.zeros((0, 3), np.int32)
    raise KeyError(name)


@pytest.mark.parametrize("name", ("s14", "s14_w3", "s11", "sphere", "zero_plane", "strip", "odd", "empty", "no_faces"))
def test_vertex_normals_equal_the_rule(env, name):
    L, ops, synthetic = env
    xyz, faces = _normal_cases(name)
    want = MR.vertex_normals(xyz, faces)
    got = ops.mesh_vertex_normals(torch.from_numpy(xyz).cuda(), torch.from_numpy(faces).cuda()).cpu().numpy()
    assert got.dtype == np.float32 and got.shape == xyz.shape
    diff = (got.view(np.uint32) != want.view(np.uint32)).any(axis=1) if len(xyz) else np.zeros(0, bool)
    assert not diff.any(), f"{int(diff.sum())} of {len(xyz)} normals differ, first at {np.flatnonzero(diff)[:1]}"
    if name == "odd":
        assert (want[3] == 0).all() and (want[4] == 0).all() and np.isfinite(want).all()
    if name == "s14_w3":
        assert ((want == 0).all(axis=1)).sum() == 1                # the vertex in no face


OPTION_SETS = {"defaults": {}, "min_faces": dict(min_component_faces=200), "fraction": dict(min_component_fraction=0.06),
               "largest": dict(keep_largest=1), "degenerate": dict(drop_degenerate=True),
               "all": dict(min_component_faces=150, min_component_fraction=0.06, keep_largest=2, drop_degenerate=True)}


def _clean_mesh(name):
    if name == "zero_plane_blobs":                                 # the zero-plane mesh twice, the copy cut short: two components, zero-area faces
        xyz, rgb, faces = MR.zero_plane_mesh()
        part = faces[:len(faces) // 3] + len(xyz)
        return np.concatenate((xyz, xyz + np.float32(9.0))), np.concatenate((rgb, rgb)), np.concatenate((faces, part))
    return MR.scene_mesh(name)[:3]


@pytest.mark.parametrize("with_normals", (False, True))
@pytest.mark.parametrize("options", list(OPTION_SETS))
@pytest.mark.parametrize("name", ("s14", "s14_w3", "zero_plane_blobs"))
def test_clean_equals_the_rule(env, name, options, with_normals):
    L, ops, synthetic = env
    xyz, rgb, faces = _clean_mesh(name)
    rgb = (np.arange(rgb.size) % 253).astype(np.uint8).reshape(rgb.shape)
    kw = dict(OPTION_SETS[options])
    if with_normals:
        kw["normals"] = MR.vertex_normals(xyz, faces)
    want = MR.clean(xyz, rgb, faces, **kw)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    got = ops.mesh_clean(dev(xyz), dev(rgb), dev(faces), **{k: (dev(v) if k == "normals" else v) for k, v in kw.items()})
    assert len(got) == len(want) == (4 if with_normals else 3)
    for g, w, what in zip(got, want, ("xyz", "rgb", "faces", "normals")):
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape, (what, g.shape, w.shape)
        np.testing.assert_array_equal(g.view(np.uint32) if g.dtype == np.float32 else g, w.view(np.uint32) if w.dtype == np.float32 else w,
                                      err_msg=what)
    # a second application equals the rule's, and changes nothing (with drop_degenerate AND a size option the components of the
    # cleaned mesh can be smaller than those of the input, which were the ones chosen from: only there may it remove more)
    again = ops.mesh_clean(*got[:3], **{k: (got[3] if k == "normals" else v) for k, v in kw.items()})
    want2 = MR.clean(*want[:3], **{k: (want[3] if k == "normals" else v) for k, v in kw.items()})
    for a, w in zip(again, want2):
        np.testing.assert_array_equal(a.cpu().numpy(), w)
    if options != "all":
        for g, a in zip(got, again):
            assert torch.equal(g, a)
    # the case does what its name says
    removed_f, removed_v = len(faces) - len(want[2]), len(xyz) - len(want[0])
    if name == "s14":
        assert (removed_f > 0) == (options in ("min_faces", "fraction", "largest", "all")) and len(want[2]) > 0
    if name == "s14_w3":
        assert removed_v == 1 and removed_f == 0                   # one component, no degenerate face: only the unused vertex goes
    if name == "zero_plane_blobs" and options in ("degenerate", "all"):
        assert removed_f >= MR.degenerate(xyz, faces[:len(MR.zero_plane_mesh()[2])]).sum() > 0


def test_clean_of_nothing_and_to_nothing(env):
    L, ops, synthetic = env
    e = lambda dt: torch.zeros((0, 3), dtype=dt, device="cuda")
    assert [tuple(a.shape) for a in ops.mesh_clean(e(torch.float32), e(torch.uint8), e(torch.int32))] == [(0, 3)] * 3
    assert [tuple(a.shape) for a in ops.mesh_clean(e(torch.float32), e(torch.uint8), e(torch.int32), normals=e(torch.float32))] == [(0, 3)] * 4
    xyz, rgb = torch.rand(5, 3, device="cuda"), torch.zeros(5, 3, dtype=torch.uint8, device="cuda")
    assert [tuple(a.shape) for a in ops.mesh_clean(xyz, rgb, e(torch.int32))] == [(0, 3)] * 3           # no face: no vertex survives
    faces = torch.tensor([[0, 1, 2], [2, 3, 4]], dtype=torch.int32, device="cuda")
    out = ops.mesh_clean(xyz, rgb, faces, min_component_faces=3, normals=xyz)
    assert [tuple(a.shape) for a in out] == [(0, 3)] * 4
    label, fcount, vcount = ops.mesh_components(e(torch.int32), 0)
    assert label.shape == fcount.shape == vcount.shape == (0,)


# ---- end to end -------------------------------------------------------------------------------------------------------------------
def test_run_cleans_the_mesh_and_the_metrics_read_its_points(env, tmp_path, monkeypatch):
    L, ops, synthetic = env
    from wild_deep_mvs_amd.evaluation import fusibile as EF, metrics as EM, tsdf_fusion as TF
    from wild_deep_mvs_amd.utils import point_cloud as PC
    V, H, W, ds = 5, 24, 32, 2
    sc = synthetic.make_fusion_scene(V, H, W)
    args = Namespace(model="vis", nviews=V, data_path=str(tmp_path), scene="sceneA_3", downscale=ds, colmap=False, filter=False,
                     prob_threshold=0.5, override=False, tsdf_voxel=0.2, tsdf_write_points=True, dataset="yfcc", override_fusion=True,
                     tsdf_keep_largest=1, tsdf_vertex_normals=True)
    folder = f"{args.model}_{args.nviews}"
    dfold = tmp_path / "IntRes" / "depthmaps" / folder / args.scene
    dfold.mkdir(parents=True)
    rng = np.random.default_rng(0)
    batches, colors = [], []
    for v in range(V):
        name = f"{v:08d}"
        np.savez(dfold / f"{name}_out.npz", depthmap=sc["depths"][v].numpy(), probability=np.ones((H, W), np.float32))
        img = torch.from_numpy(rng.random((1, V, 3, H * ds, W * ds), dtype=np.float32))
        order = [v] + [u for u in range(V) if u != v]
        Kf = sc["K"].clone()
        Kf[:, :2] *= ds
        batches.append({"filename": [name], "imgs": img, "K": Kf.unsqueeze(0)[:, order], "R": sc["R"].unsqueeze(0)[:, order],
                        "t": sc["t"].unsqueeze(0)[:, order]})
        colors.append(EF.view_colors(img[0, 0], ds))
    TF.run(batches, args)
    xyz, rgb, faces = (a.cpu().numpy() for a in TF.fuse_tsdf_mesh([d.numpy() for d in sc["depths"]], colors, sc["K"], sc["R"], sc["t"], voxel=0.2))
    want = MR.clean(xyz, rgb, faces, keep_largest=1)
    assert 0 < len(want[2]) < len(faces) and 0 < len(want[0]) < len(xyz)       # fragments were removed
    want = want + (MR.vertex_normals(want[0], want[2]),)
    got = PC.read_mesh_normals(tmp_path / "Meshes" / folder / f"{folder}{args.scene}.ply")
    for g, w, what in zip(got, want, ("xyz", "rgb", "faces", "normals")):
        np.testing.assert_array_equal(g.view(np.uint32) if g.dtype == np.float32 else g, w.view(np.uint32) if w.dtype == np.float32 else w,
                                      err_msg=what)
    # the cleaned vertices as a cloud: the metrics mirror runs on it
    cloud = PC.read_ply(tmp_path / "Points" / folder / f"{folder}{args.scene}.ply")
    np.testing.assert_array_equal(EM.format_point_cloud(cloud), want[0])
    monkeypatch.chdir(tmp_path)
    (tmp_path / "data" / "yfcc_subset_dataset" / "gt_resolution").mkdir(parents=True)
    (tmp_path / "data" / "yfcc_subset_dataset" / "gt_resolution" / "sceneA.txt").write_text("0.05\n")
    (tmp_path / "Points" / "gt").mkdir(parents=True)
    PC.write_point_cloud(tmp_path / "Points" / "gt" / "sceneA_gt.ply", want[0][::2], want[1][::2])
    EM.run(args)
    import pickle
    with open(tmp_path / "IntRes" / "chamfer" / folder / f"dists{args.scene}.pkl", "rb") as fh:
        res = pickle.load(fh)
    assert res["dist_predToGt"].shape == (len(want[0]),) and (res["dist_gtToPred"] == 0).all()
