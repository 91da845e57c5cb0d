"""CPU: the mesh clean-up rules of tests/_mesh_ref.py -- connected components with min-index labels
against scipy, the choice of the surviving components on the fusion scene's mesh (whose outlier blobs are the reason for the
step), the order-preserving compaction, degenerate faces, the float64 vertex normals -- and the host logic of the feature: the
mesh files with normals, the argument checks of the ops and of the C entry points, and run() of evaluation/tsdf_fusion.py."""
import ctypes as C
import functools
from argparse import Namespace

import numpy as np
import pytest
import torch

from tests import _mesh_ref as MR, _tsdf_ref as TR
from wild_deep_mvs_amd import _lib as L, ops, synthetic
from wild_deep_mvs_amd.evaluation import tsdf_fusion as TF
from wild_deep_mvs_amd.utils import point_cloud as PC


def scipy_labels(faces, n):
    sparse = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import connected_components
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    rows, cols = np.concatenate((f[:, 0], f[:, 0])), np.concatenate((f[:, 1], f[:, 2]))
    graph = sparse.coo_matrix((np.ones(rows.size), (rows, cols)), shape=(n, n))
    _, comp = connected_components(graph, directed=False)
    smallest = np.full(comp.max() + 1 if n else 0, n, dtype=np.int64)
    np.minimum.at(smallest, comp, np.arange(n))
    return smallest[comp].astype(np.int32)


def test_reference_labels_equal_scipy_on_random_graphs():
    rng = np.random.default_rng(0)
    for n, f in ((1, 0), (7, 3), (50, 20), (200, 60), (1000, 400), (1000, 3000)):
        faces = rng.integers(0, n, (f, 3)).astype(np.int32)
        label = MR.components(faces, n)
        np.testing.assert_array_equal(label, scipy_labels(faces, n))
        assert (label <= np.arange(n)).all() and (label[label] == label).all()
        fcount, vcount = MR.sizes(label, faces)
        assert fcount.sum() == f and vcount.sum() == n and (fcount[label != np.arange(n)] == 0).all()
    faces, n = MR.soup()
    label = MR.components(faces, n)
    np.testing.assert_array_equal(label, scipy_labels(faces, n))
    fcount, _ = MR.sizes(label, faces)
    assert 200 <= (fcount > 0).sum() <= 400                        # "a few hundred components"


@pytest.mark.parametrize("name", ("s14", "s14_w3", "s11", "sphere", "zero_plane"))
def test_reference_labels_equal_scipy_on_the_meshes(name):
    xyz, rgb, faces = (MR.sphere_mesh() if name == "sphere" else MR.zero_plane_mesh() if name == "zero_plane" else MR.scene_mesh(name))[:3]
    np.testing.assert_array_equal(MR.components(faces, len(xyz)), scipy_labels(faces, len(xyz)))


def test_the_scene_mesh_has_one_surface_and_two_outlier_blobs():
    xyz, rgb, faces, _ = MR.scene_mesh("s14")
    assert (len(xyz), len(faces)) == (2122, 3977)
    label = MR.components(faces, len(xyz))
    fcount, vcount = MR.sizes(label, faces)
    assert sorted(fcount[fcount > 0].tolist(), reverse=True) == [3569, 228, 180] and fcount.sum() == 3977
    assert vcount.sum() == 2122 and ((vcount > 0) == (label == np.arange(len(xyz)))).all()
    xyz, rgb, faces, _ = MR.scene_mesh("s11")
    fcount, _ = MR.sizes(MR.components(faces, len(xyz)), faces)
    assert (len(xyz), len(faces)) == (1964, 3705) and sorted(fcount[fcount > 0].tolist(), reverse=True) == [3519, 186]


def _n_components(faces, n):
    fcount, _ = MR.sizes(MR.components(faces, n), faces)
    return int((fcount > 0).sum())


@pytest.mark.parametrize("options, n_faces, n_comp", ((dict(min_component_faces=200), 3569 + 228, 2), (dict(keep_largest=1), 3569, 1),
                                                       (dict(min_component_fraction=0.06), 3569 + 228, 2),           # ceil(214.14) = 215
                                                       (dict(min_component_faces=229, keep_largest=2), 3569, 1)))
def test_filters_on_the_scene_mesh_remove_and_keep(options, n_faces, n_comp):
    xyz, rgb, faces, _ = MR.scene_mesh("s14")
    x2, c2, f2 = MR.clean(xyz, rgb, faces, **options)
    assert 0 < len(f2) < len(faces) and 0 < len(x2) < len(xyz)     # something is removed and something is kept
    assert len(f2) == n_faces and _n_components(f2, len(x2)) == n_comp
    assert f2.dtype == np.int32 and f2.min() == 0 and f2.max() == len(x2) - 1          # closed: every vertex is used
    # order-preserving: the output is the input with rows struck out
    label = MR.components(faces, len(xyz))
    fkeep = MR.choose(MR.sizes(label, faces)[0], **options)[label[faces[:, 0]]]
    used = np.zeros(len(xyz), dtype=bool)
    used[faces[fkeep]] = True
    np.testing.assert_array_equal(x2, xyz[used])
    np.testing.assert_array_equal(c2, rgb[used])
    np.testing.assert_array_equal(x2[f2], xyz[faces[fkeep]])
    # idempotent
    x3, c3, f3 = MR.clean(x2, c2, f2, **options)
    np.testing.assert_array_equal(x3, x2)
    np.testing.assert_array_equal(c3, c2)
    np.testing.assert_array_equal(f3, f2)


def test_the_default_call_only_drops_unused_vertices():
    xyz, rgb, faces, _ = MR.scene_mesh("s14_w3")
    assert (len(xyz), len(faces)) == (1447, 2723)
    x2, c2, f2 = MR.clean(xyz, rgb, faces)
    assert len(x2) == 1446 and len(f2) == 2723
    np.testing.assert_array_equal(x2[f2], xyz[faces])              # no face changed
    lone = np.setdiff1d(np.arange(len(xyz)), faces)
    assert len(lone) == 1
    np.testing.assert_array_equal(x2, np.delete(xyz, lone, axis=0))
    nrm = MR.vertex_normals(xyz, faces)
    x4, _, _, n4 = MR.clean(xyz, rgb, faces, normals=nrm)
    assert (nrm[lone] == 0).all() and (np.abs(np.linalg.norm(n4.astype(np.float64), axis=1) - 1.0) < 1e-6).all()
    np.testing.assert_array_equal(n4, np.delete(nrm, lone, axis=0))
    xyz, rgb, faces, _ = MR.scene_mesh("s14")                      # nothing to drop: the mesh comes back as it is
    x2, c2, f2 = MR.clean(xyz, rgb, faces)
    np.testing.assert_array_equal(x2, xyz)
    np.testing.assert_array_equal(f2, faces)


def test_keep_largest_breaks_ties_by_label():
    faces = np.array([[6, 7, 8], [0, 1, 2], [3, 4, 5], [0, 2, 9], [3, 5, 10], [6, 8, 11], [12, 13, 14]], dtype=np.int32)
    fcount, _ = MR.sizes(MR.components(faces, 15), faces)
    assert fcount[[0, 3, 6, 12]].tolist() == [2, 2, 2, 1]
    assert np.flatnonzero(MR.choose(fcount, keep_largest=1)).tolist() == [0]
    assert np.flatnonzero(MR.choose(fcount, keep_largest=2)).tolist() == [0, 3]
    assert np.flatnonzero(MR.choose(fcount, keep_largest=4)).tolist() == [0, 3, 6, 12]
    assert np.flatnonzero(MR.choose(fcount, keep_largest=99)).tolist() == [0, 3, 6, 12]          # components without a face never survive
    assert np.flatnonzero(MR.choose(fcount, min_component_faces=2, keep_largest=4)).tolist() == [0, 3, 6]
    assert np.flatnonzero(MR.choose(fcount, min_component_fraction=1.0)).tolist() == [0, 3, 6]
    xyz = np.arange(45, dtype=np.float32).reshape(15, 3) ** 1.5
    x2, _, f2 = MR.clean(xyz, np.zeros((15, 3), np.uint8), faces, keep_largest=2)
    assert f2.tolist() == [[0, 1, 2], [3, 4, 5], [0, 2, 6], [3, 5, 7]]
    np.testing.assert_array_equal(x2, xyz[[0, 1, 2, 3, 4, 5, 9, 10]])


def test_drop_degenerate():
    xyz, rgb, faces = MR.zero_plane_mesh()
    bad = MR.degenerate(xyz, faces)
    assert 0 < bad.sum() < len(faces)
    x2, c2, f2 = MR.clean(xyz, rgb, faces, drop_degenerate=True)
    assert len(f2) == len(faces) - bad.sum() and not MR.degenerate(x2, f2).any()
    for got, want in zip(MR.clean(x2, c2, f2, drop_degenerate=True), (x2, c2, f2)):              # idempotent
        np.testing.assert_array_equal(got, want)
    assert len(MR.clean(xyz, rgb, faces)[2]) == len(faces)
    xyz, rgb, faces = MR.sphere_mesh()
    assert not MR.degenerate(xyz, faces).any()
    assert len(MR.clean(xyz, rgb, faces, drop_degenerate=True)[2]) == len(faces)
    assert MR.degenerate(xyz, np.array([[0, 5, 0], [1, 1, 1], [0, 1, 2]], dtype=np.int32)).tolist() == [True, True, False]


def test_sphere_normals_are_unit_and_point_outwards():
    xyz, rgb, faces = MR.sphere_mesh()
    nrm = MR.vertex_normals(xyz, faces)
    assert nrm.dtype == np.float32 and nrm.shape == xyz.shape
    assert (np.abs(np.linalg.norm(nrm.astype(np.float64), axis=1) - 1.0) < 1e-6).all()
    centre = np.array(MR.SPHERE_ORIGIN) + (MR.SPHERE_N - 1) / 2.0
    radial = xyz.astype(np.float64) - centre
    cosine = np.einsum("ij,ij->i", nrm, radial) / np.linalg.norm(radial, axis=1)
    assert (cosine > 0.0).all() and np.median(cosine) > 0.98


def test_scene_normals_face_the_cameras():
    xyz, rgb, faces, sc = MR.scene_mesh("s14")
    x2, c2, f2 = MR.clean(xyz, rgb, faces, keep_largest=1)         # (the outlier blobs are closed: their far sides face away)
    nrm = MR.vertex_normals(x2, f2).astype(np.float64)
    assert (np.abs(np.linalg.norm(nrm, axis=1) - 1.0) < 1e-6).all()
    R, t = sc["R"].numpy().astype(np.float64), sc["t"].numpy().astype(np.float64)
    for v in range(R.shape[0]):
        centre = -(R[v].T @ t[v]).reshape(3)
        assert (np.einsum("ij,ij->i", nrm, centre - x2.astype(np.float64)) > 0.0).all(), v
    assert np.median(nrm @ sc["n"]) < -0.95                         # the plane's normal, towards the cameras at z = 0


def test_normals_of_odd_faces():
    xyz = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [5, 5, 5], [2, 0, 0], [0, 0, 1]], dtype=np.float32)
    faces = np.array([[0, 1, 2], [0, 1, 4], [0, 0, 5], [1, 2, 5]], dtype=np.int32)           # a zero-area face, a repeated index
    nrm = MR.vertex_normals(xyz, faces)
    assert nrm[3].tolist() == [0, 0, 0] and nrm[4].tolist() == [0, 0, 0] and nrm[0].tolist() == [0, 0, 1]
    assert abs(float(np.linalg.norm(nrm[5].astype(np.float64))) - 1.0) < 1e-6
    assert MR.vertex_normals(xyz[:0], faces[:0]).shape == (0, 3) and (MR.vertex_normals(xyz, faces[:0]) == 0).all()


# ---- files ------------------------------------------------------------------------------------------------------------------------
def test_mesh_files_with_and_without_normals(tmp_path):
    xyz, rgb, faces = MR.sphere_mesh()
    rgb = (np.arange(rgb.size) % 251).astype(np.uint8).reshape(rgb.shape)
    nrm = MR.vertex_normals(xyz, faces)
    path = tmp_path / "mesh.ply"
    PC.write_mesh(path, torch.from_numpy(xyz), rgb, faces, torch.from_numpy(nrm))
    head = path.read_bytes().split(b"end_header\n")[0].decode().split("\n")
    assert head[3:12] == [f"property float32 {c}" for c in ("x", "y", "z", "nx", "ny", "nz")] + [f"property uint8 {c}" for c in ("red", "green", "blue")]
    x2, c2, f2, n2 = PC.read_mesh_normals(path)
    assert n2.dtype == np.float32
    for got, want in ((x2, xyz), (c2, rgb), (f2, faces), (n2, nrm)):
        np.testing.assert_array_equal(got, want)
    three = PC.read_mesh(path)                                     # the three-tuple reader reads the new file too
    assert len(three) == 3
    for got, want in zip(three, (xyz, rgb, faces)):
        np.testing.assert_array_equal(got, want)
    with pytest.raises(ValueError, match="normals"):
        PC.write_mesh(path, xyz, rgb, faces, nrm[:-1])
    # without normals: the bytes of the writer before normals existed, restated here
    PC.write_mesh(path, xyz, rgb, faces)
    vertex = np.empty(len(xyz), dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
    for k, c in enumerate("xyz"):
        vertex[c] = xyz[:, k]
    for k, c in enumerate(("red", "green", "blue")):
        vertex[c] = rgb[:, k]
    face = np.empty(len(faces), dtype=[("n", "u1"), ("v", "<i4", (3,))])
    face["n"], face["v"] = 3, faces
    header = PC.mesh_ply_header(len(xyz), len(faces))
    assert b"nx" not in header and header.count(b"property") == 7
    assert path.read_bytes() == header + vertex.tobytes() + face.tobytes()
    x2, c2, f2, n2 = PC.read_mesh_normals(path)
    assert n2 is None and len(x2) == len(xyz)
    PC.write_mesh(path, xyz[:0], rgb[:0], faces[:0], nrm[:0])
    assert [a.shape for a in PC.read_mesh_normals(path)] == [(0, 3)] * 4


# ---- argument checks --------------------------------------------------------------------------------------------------------------
def test_ops_check_their_arguments_before_any_launch():
    xyz, rgb = torch.zeros(5, 3), torch.zeros(5, 3, dtype=torch.uint8)
    faces = torch.tensor([[0, 1, 2], [2, 3, 4]], dtype=torch.int32)
    for bad in (faces.long(), faces.reshape(-1), faces[:, :2], faces.numpy(), None):
        with pytest.raises(ValueError, match="pscv.mesh_components: faces"):
            ops.mesh_components(bad, 5)
    for bad in (-1, 2.5, True, None, 2 ** 31):
        with pytest.raises(ValueError, match="pscv.mesh_components: (n_vertices|.* do not fit)"):
            ops.mesh_components(faces, bad)
    with pytest.raises(ValueError, match="pscv.mesh_components: faces must be on the GPU"):
        ops.mesh_components(faces, 5)
    with pytest.raises(ValueError, match="pscv.mesh_vertex_normals: xyz"):
        ops.mesh_vertex_normals(xyz.double(), faces)
    with pytest.raises(ValueError, match="pscv.mesh_vertex_normals: xyz"):
        ops.mesh_vertex_normals(xyz[:, :2], faces)
    with pytest.raises(ValueError, match="pscv.mesh_vertex_normals: faces"):
        ops.mesh_vertex_normals(xyz, faces.long())
    with pytest.raises(ValueError, match="pscv.mesh_vertex_normals: xyz must be on the GPU"):
        ops.mesh_vertex_normals(xyz, faces)
    for change, word in ((dict(xyz=xyz.half()), "xyz"), (dict(rgb=rgb.float()), "rgb"), (dict(rgb=rgb[:4]), "rgb"), (dict(rgb=None), "rgb"),
                         (dict(faces=faces.long()), "faces"), (dict(normals=xyz[:4]), "normals"), (dict(normals=xyz.double()), "normals"),
                         (dict(min_component_faces=-1), "min_component_faces"), (dict(min_component_faces=1.5), "min_component_faces"),
                         (dict(keep_largest=-2), "keep_largest"), (dict(keep_largest=True), "keep_largest"),
                         (dict(min_component_fraction=-0.1), "min_component_fraction"), (dict(min_component_fraction=1.5), "min_component_fraction"),
                         (dict(min_component_fraction=float("nan")), "min_component_fraction"), (dict(min_component_fraction="a"), "min_component_fraction"),
                         (dict(drop_degenerate=1), "drop_degenerate")):
        args = dict(dict(xyz=xyz, rgb=rgb, faces=faces), **change)
        with pytest.raises(ValueError, match=f"pscv.mesh_clean: {word}"):
            ops.mesh_clean(args.pop("xyz"), args.pop("rgb"), args.pop("faces"), **args)
    with pytest.raises(ValueError, match="pscv.mesh_clean: xyz must be on the GPU"):       # valid arguments: there is no CPU path
        ops.mesh_clean(xyz, rgb, faces, min_component_faces=3, min_component_fraction=0.5, keep_largest=1, drop_degenerate=True, normals=xyz)


def test_exports_and_c_argument_checks():
    vp, i, l = C.c_void_p, C.c_int, C.c_long
    assert L.PROTOTYPES["pscv_mesh_components"] == (i, [vp, l, l, vp, vp, vp])
    assert L.PROTOTYPES["pscv_mesh_component_sizes"] == (i, [vp, vp, l, l, vp, vp, vp])
    assert L.PROTOTYPES["pscv_mesh_mark"] == (i, [vp, vp, vp, vp, l, l, i, vp, vp, vp])
    assert L.PROTOTYPES["pscv_mesh_compact"] == (i, [vp] * 8 + [l, l] + [vp] * 4 + [l, l, vp])
    assert L.PROTOTYPES["pscv_mesh_vertex_normals"] == (i, [vp, vp, vp, vp, l, l, vp, vp])
    assert L.ABI_VERSION == 14
    try:
        lib = L.lib()
    except L.PscvMissingError:
        pytest.skip("libpscv.so is not built")
    a = 64                                   # a non-null address; every call below is refused, or has nothing to do, before it is used
    big, third = 2 ** 31, (2 ** 31 - 1) // 3 + 1
    err = lib.pscv_last_error
    assert lib.pscv_mesh_components(a, 2, -1, a, a, None) == -1 and b"n_vertices" in err()
    assert lib.pscv_mesh_components(a, 2, big, a, a, None) == -1 and b"n_vertices" in err()
    assert lib.pscv_mesh_components(a, -1, 5, a, a, None) == -1 and b"n_faces" in err()
    assert lib.pscv_mesh_components(a, third, 5, a, a, None) == -1 and b"n_faces" in err()
    assert lib.pscv_mesh_components(a, 2, 5, a, None, None) == -1 and b"null" in err()
    assert lib.pscv_mesh_components(a, 2, 5, None, a, None) == -1 and b"null" in err()
    assert lib.pscv_mesh_components(None, 2, 5, a, a, None) == -1 and b"null" in err()
    assert lib.pscv_mesh_components(None, 0, 0, None, a, None) == 0                            # nothing to launch
    assert lib.pscv_mesh_component_sizes(a, a, 2, big, a, a, None) == -1 and b"n_vertices" in err()
    assert lib.pscv_mesh_component_sizes(a, a, 2, 5, None, a, None) == -1 and b"null" in err()
    assert lib.pscv_mesh_component_sizes(a, None, 2, 5, a, a, None) == -1 and b"null" in err()
    assert lib.pscv_mesh_component_sizes(None, None, 0, 0, None, None, None) == 0
    assert lib.pscv_mesh_mark(a, a, a, a, 2, 5, 2, a, a, None) == -1 and b"drop_degenerate" in err()
    assert lib.pscv_mesh_mark(a, a, a, a, -2, 5, 0, a, a, None) == -1 and b"n_faces" in err()
    assert lib.pscv_mesh_mark(a, a, a, a, 2, 5, 0, None, a, None) == -1 and b"null" in err()
    assert lib.pscv_mesh_mark(a, a, a, None, 2, 5, 0, a, a, None) == -1 and b"null" in err()
    assert lib.pscv_mesh_mark(None, None, None, None, 0, 5, 1, None, None, None) == 0
    ok = [a, a, None, a, a, a, a, a, 2, 5, a, a, None, a, 2, 5]
    for change, word in (({14: 3}, b"n_faces_out"), ({14: -1}, b"n_faces_out"), ({15: 6}, b"n_vertices_out"), ({9: big}, b"n_vertices"),
                         ({2: a}, b"normals"), ({12: a}, b"normals"), ({0: None}, b"null"), ({7: None}, b"null"), ({10: None}, b"null"),
                         ({13: None}, b"null"), ({4: None}, b"null")):
        args = list(ok)
        for k, v in change.items():
            args[k] = v
        assert lib.pscv_mesh_compact(*args, None) == -1 and word in err(), word
    assert lib.pscv_mesh_compact(*([None] * 8 + [2, 5] + [None] * 4 + [0, 0]), None) == 0      # nothing survives: nothing to launch
    assert lib.pscv_mesh_vertex_normals(a, a, a, a, 2, -5, a, None) == -1 and b"n_vertices" in err()
    assert lib.pscv_mesh_vertex_normals(a, a, None, a, 2, 5, a, None) == -1 and b"null" in err()
    assert lib.pscv_mesh_vertex_normals(a, a, a, None, 2, 5, a, None) == -1 and b"null" in err()
    assert lib.pscv_mesh_vertex_normals(a, a, a, a, 2, 5, None, None) == -1 and b"null" in err()
    assert lib.pscv_mesh_vertex_normals(None, None, None, None, 0, 0, None, None) == 0


# ---- run() ------------------------------------------------------------------------------------------------------------------------
def _fake_ops(monkeypatch, seen):
    """The five ops of run() replaced by the numpy rules, on CPU tensors."""
    def fake_integrate(state, depths, colors, cams, *, origin, voxel, trunc):
        TR.integrate(state, [d.numpy() for d in depths], [c.numpy() for c in colors], cams.numpy(), origin, voxel, trunc)

    def fake_extract(state, *, origin, voxel, min_weight):
        return tuple(torch.from_numpy(a) for a in TR.extract(state, origin, voxel, min_weight))

    def fake_clean(xyz, rgb, faces, **options):
        seen.append(("clean", options))
        return tuple(torch.from_numpy(a) for a in MR.clean(xyz.numpy(), rgb.numpy(), faces.numpy(), **options))

    def fake_normals(xyz, faces):
        seen.append(("normals", len(xyz)))
        return torch.from_numpy(MR.vertex_normals(xyz.numpy(), faces.numpy()))

    monkeypatch.setattr(TF.ops, "tsdf_volume", lambda dims, device: TR.volume(dims))
    monkeypatch.setattr(TF.ops, "tsdf_integrate", fake_integrate)
    monkeypatch.setattr(TF.ops, "tsdf_extract", fake_extract)
    monkeypatch.setattr(TF.ops, "mesh_clean", fake_clean)
    monkeypatch.setattr(TF.ops, "mesh_vertex_normals", fake_normals)
    monkeypatch.setattr(TF, "fuse_tsdf_mesh", functools.partial(TF.fuse_tsdf_mesh, device="cpu"))


def test_clean_options():
    assert TF.clean_options(Namespace()) == {}
    assert TF.clean_options(Namespace(tsdf_min_component_faces=None, tsdf_min_component_fraction=None, tsdf_keep_largest=None,
                                      tsdf_drop_degenerate=None, tsdf_vertex_normals=None, tsdf_voxel=0.1)) == {}
    assert TF.clean_options(Namespace(tsdf_drop_degenerate=False, tsdf_vertex_normals=False)) == {}
    assert TF.clean_options(Namespace(tsdf_min_component_faces=0)) == dict(min_component_faces=0)
    assert TF.clean_options(Namespace(tsdf_min_component_faces=50, tsdf_min_component_fraction=0.1, tsdf_keep_largest=2,
                                      tsdf_drop_degenerate=True, tsdf_vertex_normals=True)) == \
        dict(min_component_faces=50, min_component_fraction=0.1, keep_largest=2, drop_degenerate=True, vertex_normals=True)


def test_run_cleans_only_when_asked(tmp_path, monkeypatch):
    """run() with the ops replaced by the numpy rules: with no clean-up argument the two files are the bytes of the path without
    the step (the extracted mesh handed to the writers as it is); with arguments they are clean_mesh of the reference."""
    V, H, W, ds = 5, 24, 32, 2
    sc = synthetic.make_fusion_scene(V, H, W)
    base = dict(model="mvsnet", nviews=V, data_path=str(tmp_path), scene="scan1", downscale=ds, colmap=False, filter=False,
                prob_threshold=0.5, override=True, tsdf_voxel=0.2, tsdf_write_points=True)
    folder = f"mvsnet_{V}"
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
    seen = []
    _fake_ops(monkeypatch, seen)
    mesh_file = tmp_path / "Meshes" / folder / f"{folder}scan1.ply"
    cloud_file = tmp_path / "Points" / folder / f"{folder}scan1.ply"
    # no argument: the step does not run, and the files are what the writers make of the extracted mesh
    TF.run(batches, Namespace(**base))
    assert seen == []
    from wild_deep_mvs_amd.evaluation.fusibile import masked_view
    views = [masked_view(Namespace(**base), b, dfold) for b in batches]
    depths, colors, K, R, t = zip(*views)
    xyz, rgb, faces = (a.numpy() for a in TF.fuse_tsdf_mesh(depths, colors, torch.stack(K), torch.stack(R), torch.stack(t), voxel=0.2))
    PC.write_mesh(tmp_path / "want.ply", xyz, rgb, faces)
    PC.write_point_cloud(tmp_path / "want_points.ply", xyz, rgb)
    assert mesh_file.read_bytes() == (tmp_path / "want.ply").read_bytes()
    assert cloud_file.read_bytes() == (tmp_path / "want_points.ply").read_bytes()
    TF.run(batches, Namespace(**base, tsdf_min_component_faces=None, tsdf_keep_largest=None, tsdf_vertex_normals=False))
    assert seen == [] and mesh_file.read_bytes() == (tmp_path / "want.ply").read_bytes()
    fcount, _ = MR.sizes(MR.components(faces, len(xyz)), faces)
    assert (fcount > 0).sum() >= 2                                 # the mesh has fragments to remove
    # with arguments
    TF.run(batches, Namespace(**base, tsdf_keep_largest=1, tsdf_min_component_faces=10, tsdf_drop_degenerate=True, tsdf_vertex_normals=True))
    assert seen[0] == ("clean", dict(min_component_faces=10, min_component_fraction=0.0, keep_largest=1, drop_degenerate=True))
    want = MR.clean(xyz, rgb, faces, keep_largest=1, min_component_faces=10, drop_degenerate=True)
    assert seen[1] == ("normals", len(want[0])) and 0 < len(want[2]) < len(faces)
    got = PC.read_mesh_normals(mesh_file)
    for g, w in zip(got, want + (MR.vertex_normals(want[0], want[2]),)):
        np.testing.assert_array_equal(g, w)
    cloud = PC.read_ply(cloud_file)                                # the cloud is the cleaned vertices
    np.testing.assert_array_equal(np.stack([cloud[c] for c in "xyz"], axis=1), want[0])
    # cleaning without normals writes the old vertex layout
    TF.run(batches, Namespace(**base, tsdf_min_component_fraction=0.5))
    got = PC.read_mesh_normals(mesh_file)
    assert got[3] is None
    for g, w in zip(got, MR.clean(xyz, rgb, faces, min_component_fraction=0.5)):
        np.testing.assert_array_equal(g, w)
