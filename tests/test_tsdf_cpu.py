"""CPU: the TSDF integration and marching-tetrahedra rules of tests/_tsdf_ref.py on an analytic sphere
and on the fusion scene's plane, the face kernel's case table against the lattice rule, the mesh files, and the host logic of the
feature (argument checks of the ops and of the C entry points, the grid guard and run() of evaluation/tsdf_fusion.py).

The plane bars.  Each is twice the maximum distance of this file's reference from the scene's plane, measured on the same scene and
grid (PLANE_CASES holds the measured figure; the factor 2 is the issue's).  The scenes are make_fusion_scene(4, 24, 32, exact=True)
and (9, 48, 64, exact=True), which use no random numbers.  Two grids each, trunc = 3 voxels:
  * the mirror's default grid (voxel = two pixel footprints, bounds = the unprojected pixels padded by trunc): 25 x 21 x 10 of
    0.2776 and 45 x 38 x 13 of 0.1390; measured 0.02637 and 0.04249 voxel, bars 0.0527 and 0.0850;
  * the shapes of the rule's prototype, centred on the unprojected pixels: 35 x 29 x 11 of 0.2 and 47 x 40 x 13 of the default
    0.1390; measured 0.04371 and 0.04264 voxel, bars 0.0874 and 0.0853 (the prototype's own placement is not known: it reported
    0.050 and 0.034)."""
import ctypes as C
import functools
from argparse import Namespace

import numpy as np
import pytest
import torch

from tests import _tsdf_ref as TR
from wild_deep_mvs_amd import _lib as L, ops, synthetic
from wild_deep_mvs_amd.evaluation import tsdf_fusion as TF
from wild_deep_mvs_amd.utils import point_cloud as PC

# name: (scene, dims, voxel or None = the mirror's default, True = the mirror's padded bounds / False = centred, measured maximum)
PLANE_CASES = {"v4": ((4, 24, 32), (25, 21, 10), None, True, 0.02637), "v9": ((9, 48, 64), (45, 38, 13), None, True, 0.04249),
               "v4_35x29x11": ((4, 24, 32), (35, 29, 11), 0.2, False, 0.04371), "v9_47x40x13": ((9, 48, 64), (47, 40, 13), None, False, 0.04264)}


def sphere_state(n=14, radius=4.7, origin=(0.013, 0.027, 0.041)):
    """An n^3 grid of unit voxels holding the distance to a sphere about the grid's centre, offset so that no value is 0."""
    st = TR.volume((n, n, n))
    X, Y, Z = TR.lattice((n, n, n), origin, 1.0)
    c = (n - 1) / 2.0
    f = np.sqrt((X - c - origin[0]) ** 2 + (Y - c - origin[1]) ** 2 + (Z - c - origin[2]) ** 2) - radius
    st["tsdf_sum"][...] = f.astype(np.float32)
    st["weight"][...] = 1
    assert (st["tsdf_sum"] != 0).all()
    return st, origin


def n_undirected(faces):
    return len(np.unique(np.sort(TR.directed_edges(faces), axis=1), axis=0))


def test_sphere_is_a_closed_outward_surface():
    st, origin = sphere_state()
    xyz, rgb, faces = TR.extract(st, origin, 1.0)
    assert len(xyz) > 500 and len(faces) > 1000
    assert len(TR.unmatched_edges(faces)) == 0                     # every directed edge is matched once by its reverse
    assert len(xyz) - n_undirected(faces) + len(faces) == 2
    assert TR.signed_volume(xyz, faces) > 0.0
    p = xyz.astype(np.float64)
    nrm = np.cross(p[faces[:, 1]] - p[faces[:, 0]], p[faces[:, 2]] - p[faces[:, 0]])
    centre = np.array(origin) + 6.5
    out = np.einsum("ij,ij->i", nrm, p[faces].mean(axis=1) - centre)
    assert (out[np.linalg.norm(nrm, axis=1) > 1e-12] > 0.0).all()  # every face normal points to the positive side
    assert (rgb == 0).all()                                        # no colour was integrated


@pytest.fixture(scope="module", params=list(PLANE_CASES))
def plane(request):
    (V, H, W), dims, voxel, padded, measured = PLANE_CASES[request.param]
    bar = 2 * measured
    sc = synthetic.make_fusion_scene(V, H, W, exact=True)
    voxel = TF.default_voxel(sc["depths"], sc["K"]) if voxel is None else voxel
    trunc = 3 * voxel
    lo, hi = TF.world_bounds(sc["depths"], sc["K"], sc["R"], sc["t"])
    if padded:
        lo, hi = tuple(v - trunc for v in lo), tuple(v + trunc for v in hi)
        assert TF.grid_dims(lo, hi, voxel) == dims
    else:
        lo = tuple((a + b) / 2 - (n - 1) / 2 * voxel for a, b, n in zip(lo, hi, dims))
    cams = ops.geo_filter_cams(sc["K"], sc["R"], sc["t"]).numpy()
    st = TR.integrate(TR.volume(dims), [d.numpy() for d in sc["depths"]], [c.numpy() for c in sc["colors"]], cams, lo, voxel, trunc)
    return sc, st, lo, voxel, bar, TR.extract(st, lo, voxel)


def test_plane_vertices_lie_on_the_plane(plane):
    sc, st, lo, voxel, bar, (xyz, rgb, faces) = plane
    dist = np.abs(xyz.astype(np.float64) @ sc["n"] - sc["c0"]) / voxel
    print(f"max distance to the plane: {dist.max():.5f} voxel (bar {bar:.4f})")
    assert len(xyz) > 500 and dist.max() <= bar
    # colours: the texture is a function of the world position, so a vertex's colour is close to the texture there
    X = xyz.astype(np.float64)
    tex = np.stack((128 + 100 * np.sin(3.1 * X[:, 0]), 128 + 100 * np.sin(2.3 * X[:, 1] + 1.0), 128 + 100 * np.cos(1.7 * (X[:, 0] + X[:, 1]))), -1)
    assert np.median(np.abs(rgb.astype(np.float64) - tex)) < 12.0


def test_plane_faces_face_the_cameras(plane):
    sc, st, lo, voxel, bar, (xyz, rgb, faces) = plane
    p = xyz.astype(np.float64)
    nrm = np.cross(p[faces[:, 1]] - p[faces[:, 0]], p[faces[:, 2]] - p[faces[:, 0]])
    keep = np.linalg.norm(nrm, axis=1) > 1e-12
    centroid = p[faces].mean(axis=1)
    R, t = sc["R"].numpy().astype(np.float64), sc["t"].numpy().astype(np.float64)
    for v in range(R.shape[0]):
        centre = -(R[v].T @ t[v]).reshape(3)
        assert (np.einsum("ij,ij->i", nrm, centre - centroid)[keep] > 0.0).all(), v


def test_plane_mesh_is_open_only_at_its_boundary(plane):
    sc, st, lo, voxel, bar, (xyz, rgb, faces) = plane
    e = TR.directed_edges(faces)
    n = len(xyz)
    key = e[:, 0] * n + e[:, 1]
    assert len(np.unique(key)) == len(key)                         # no directed edge twice: at most two faces per edge, opposed
    lone = TR.unmatched_edges(faces)
    assert 0 < len(lone) < len(e) // 10
    # a lone edge lies where the surface leaves the observed region: next to an unobserved voxel or the grid's border
    obs = st["weight"] >= 1
    nz, ny, nx = obs.shape
    pad = np.zeros((nz + 4, ny + 4, nx + 4), dtype=bool)
    pad[2:-2, 2:-2, 2:-2] = obs
    ijk = np.floor((xyz.astype(np.float64) - np.array(lo)) / voxel + 1e-6).astype(int)
    for a in np.unique(lone):
        i, j, k = ijk[a]
        assert not pad[k + 1:k + 5, j + 1:j + 5, i + 1:i + 5].all(), (a, i, j, k)


def test_case_table_is_the_lattice_rule():
    tab = (C.c_uint * 96)()
    assert L.lib().pscv_tsdf_case_table(tab) == 0
    want = TR.case_table()
    for T in range(6):
        for neg in range(16):
            assert tab[T * 16 + neg] == want[T * 16 + neg], (T, neg)
    assert L.lib().pscv_tsdf_case_table(None) == -1
    # the rule itself: a cycle exists exactly for mixed signs and is reversed when the signs are
    for T in range(6):
        for neg in range(1, 15):
            a, b = TR.tet_case(T, neg), TR.tet_case(T, 15 - neg)
            assert len(a) == (4 if bin(neg).count("1") == 2 else 3) and set(a) == set(b)
            k = b.index(a[0])
            assert tuple(b[(k - n) % len(b)] for n in range(len(b))) == a
        assert TR.tet_case(T, 0) == () and TR.tet_case(T, 15) == ()


def test_mesh_file_round_trip(tmp_path):
    st, origin = sphere_state(8, 2.6)
    xyz, rgb, faces = TR.extract(st, origin, 1.0)
    rgb = (np.arange(rgb.size) % 251).astype(np.uint8).reshape(rgb.shape)
    path = tmp_path / "mesh.ply"
    PC.write_mesh(path, torch.from_numpy(xyz), rgb, faces)
    head = path.read_bytes().split(b"end_header\n")[0].decode()
    assert "format binary_little_endian 1.0" in head and f"element face {len(faces)}" in head
    assert "property list uchar int vertex_indices" in head
    x2, c2, f2 = PC.read_mesh(path)
    assert x2.dtype == np.float32 and c2.dtype == np.uint8 and f2.dtype == np.int32
    np.testing.assert_array_equal(x2, xyz)
    np.testing.assert_array_equal(c2, rgb)
    np.testing.assert_array_equal(f2, faces)
    PC.write_mesh(path, xyz[:0], rgb[:0], faces[:0])                # an empty mesh is a file too
    assert [a.shape for a in PC.read_mesh(path)] == [(0, 3), (0, 3), (0, 3)]
    with pytest.raises(ValueError, match="face indices"):
        PC.write_mesh(path, xyz, rgb, faces + len(xyz))
    with pytest.raises(ValueError, match="rgb"):
        PC.write_mesh(path, xyz, rgb.astype(np.int32), faces)
    with pytest.raises(ValueError, match="faces"):
        PC.write_mesh(path, xyz, rgb, faces.astype(np.float32))
    PC.write_point_cloud(path, xyz, rgb)
    with pytest.raises(ValueError, match="element face"):
        PC.read_mesh(path)


def test_ops_check_their_arguments_on_cpu_tensors():
    with pytest.raises(ValueError, match="pscv.tsdf_volume: dims"):
        ops.tsdf_volume((0, 2, 2), "cpu")
    with pytest.raises(ValueError, match="pscv.tsdf_volume: dims"):
        ops.tsdf_volume((2048, 2048, 512), "cpu")
    with pytest.raises(ValueError, match="pscv.tsdf_volume: dims"):
        ops.tsdf_volume((2, 2), "cpu")
    st = ops.tsdf_volume((4, 3, 2), "cpu")
    assert st.tsdf_sum.shape == (2, 3, 4) and st.rgb_sum.shape == (2, 3, 4, 3) and st.weight.dtype == torch.int32
    assert all(int(a.abs().sum()) == 0 for a in st.arrays()) and st.views == 0
    depths, colors = [torch.ones(5, 7)], [torch.zeros(5, 7, 3, dtype=torch.uint8)]
    cams = ops.geo_filter_cams(torch.eye(3)[None], torch.eye(3)[None], torch.zeros(1, 3, 1))
    good = dict(origin=(0.0, 0.0, 0.0), voxel=0.5, trunc=1.5)
    for bad, word in ((dict(origin=(0.0, 0.0)), "origin"), (dict(origin=(0.0, float("nan"), 0.0)), "origin"), (dict(voxel=0.0), "voxel"),
                      (dict(voxel=float("inf")), "voxel"), (dict(trunc=-1.0), "trunc"), (dict(trunc=float("nan")), "trunc")):
        with pytest.raises(ValueError, match=f"pscv.tsdf_integrate: {word}"):
            ops.tsdf_integrate(st, depths, colors, cams, **dict(good, **bad))
    with pytest.raises(ValueError, match="state must be"):
        ops.tsdf_integrate({"tsdf_sum": st.tsdf_sum}, depths, colors, cams, **good)
    with pytest.raises(ValueError, match="state.weight"):
        ops.tsdf_integrate(ops.TsdfVolume(st.dims, st.tsdf_sum, st.weight.long(), st.rgb_sum, st.cweight), depths, colors, cams, **good)
    with pytest.raises(ValueError, match="as many colour"):
        ops.tsdf_integrate(st, depths, [], cams, **good)
    with pytest.raises(ValueError, match="at least one"):
        ops.tsdf_integrate(st, [], [], cams, **good)
    with pytest.raises(ValueError, match="colours of view 0"):
        ops.tsdf_integrate(st, depths, [torch.zeros(5, 6, 3, dtype=torch.uint8)], cams, **good)
    with pytest.raises(ValueError, match="depth map 0"):
        ops.tsdf_integrate(st, [torch.ones(5, 7, dtype=torch.float64)], colors, cams, **good)
    with pytest.raises(ValueError, match="cams"):
        ops.tsdf_integrate(st, depths, colors, cams[:, :29], **good)
    full = ops.TsdfVolume(st.dims, *st.arrays(), views=ops.TSDF_MAX_VIEWS)
    with pytest.raises(ValueError, match="exceed the 65793"):
        ops.tsdf_integrate(full, depths, colors, cams, **good)
    with pytest.raises(RuntimeError, match="no CPU"):                       # valid arguments: there is no CPU path
        ops.tsdf_integrate(st, depths, colors, cams, **good)
    assert st.views == 0
    for bad, word in ((dict(min_weight=0), "min_weight"), (dict(min_weight=1.5), "min_weight"), (dict(voxel=-1.0), "voxel"),
                      (dict(origin="abc"), "origin")):
        with pytest.raises(ValueError, match=f"pscv.tsdf_extract: {word}"):
            ops.tsdf_extract(st, **dict(dict(origin=(0.0, 0.0, 0.0), voxel=0.5), **bad))
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.tsdf_extract(st, origin=(0.0, 0.0, 0.0), voxel=0.5)


def test_exports_and_c_argument_checks():
    vp, i, l, d = C.c_void_p, C.c_int, C.c_long, C.c_double
    pp = C.POINTER(vp)
    assert L.PROTOTYPES["pscv_tsdf_integrate"] == (i, [pp, pp, vp, i, vp, vp, d, d, d, d, d, i, i, i, vp, vp, vp, vp, vp])
    assert L.PROTOTYPES["pscv_tsdf_mark"] == (i, [vp, vp, i, i, i, i, vp, vp])
    assert L.PROTOTYPES["pscv_tsdf_emit_vertices"] == (i, [vp, vp, vp, vp, vp, vp, i, i, i, d, d, d, d, vp, vp, l, vp])
    assert L.PROTOTYPES["pscv_tsdf_emit_faces"] == (i, [vp, vp, vp, i, i, i, vp, l, vp])
    assert L.ABI_VERSION == 14
    lib = L.lib()
    one = (vp * 1)(64)                       # a non-null address; every call below is refused before it is used
    hw = (C.c_int * 2)(5, 7)
    nan, inf = float("nan"), float("inf")
    ok = [one, one, hw, 1, 64, 64, 0.0, 0.0, 0.0, 0.5, 1.5, 4, 3, 2, 64, 64, 64, 64]
    cases = [({0: None}, b"null"), ({14: None}, b"null"), ({3: 0}, b"n_views"), ({3: 65}, b"n_views"), ({6: nan}, b"origin"),
             ({8: inf}, b"origin"), ({9: 0.0}, b"voxel"), ({9: nan}, b"voxel"), ({10: 0.0}, b"trunc"), ({10: inf}, b"trunc"),
             ({11: 0}, b"dims"), ({11: 65536, 12: 65536, 13: 1}, b"dims"), ({11: 2048, 12: 2048, 13: 512}, b"dims"),
             ({2: (C.c_int * 2)(5, 0)}, b"bad size"), ({1: (vp * 1)(None)}, b"view 0 has a null pointer")]
    for change, word in cases:
        args = list(ok)
        for k, v in change.items():
            args[k] = v
        assert lib.pscv_tsdf_integrate(*args, None) == -1 and word in lib.pscv_last_error(), word
    assert lib.pscv_tsdf_mark(None, 64, 4, 3, 2, 1, 64, None) == -1 and b"null" in lib.pscv_last_error()
    assert lib.pscv_tsdf_mark(64, 64, 4, 3, 2, 0, 64, None) == -1 and b"min_weight" in lib.pscv_last_error()
    assert lib.pscv_tsdf_mark(64, 64, 4, -3, 2, 1, 64, None) == -1 and b"dims" in lib.pscv_last_error()
    ev = [64, 64, 64, 64, 64, 64, 4, 3, 2, 0.0, 0.0, 0.0, 0.5, 64, 64, 5]
    for change, word in (({15: -1}, b"n_vertices"), ({15: 2 ** 31}, b"n_vertices"), ({12: 0.0}, b"voxel"), ({9: inf}, b"origin"),
                         ({8: 0}, b"dims"), ({13: None}, b"null"), ({5: None}, b"null")):
        args = list(ev)
        for k, v in change.items():
            args[k] = v
        assert lib.pscv_tsdf_emit_vertices(*args, None) == -1 and word in lib.pscv_last_error(), word
    assert lib.pscv_tsdf_emit_vertices(*(ev[:13] + [None, None, 0]), None) == 0           # no vertices: nothing to launch
    assert lib.pscv_tsdf_emit_faces(64, 64, 64, 4, 3, 2, 64, -1, None) == -1 and b"n_faces" in lib.pscv_last_error()
    assert lib.pscv_tsdf_emit_faces(64, 64, 64, 4, 3, 0, 64, 5, None) == -1 and b"dims" in lib.pscv_last_error()
    assert lib.pscv_tsdf_emit_faces(64, 64, None, 4, 3, 2, 64, 5, None) == -1 and b"null" in lib.pscv_last_error()
    assert lib.pscv_tsdf_emit_faces(None, None, None, 4, 3, 2, None, 0, None) == 0


def test_grid_guard_names_the_grid():
    sc = synthetic.make_fusion_scene(4, 24, 32, exact=True)
    with pytest.raises(ValueError, match=r"25 x 21 x 10 voxels .* max_voxels = 5000: pass `bounds` or a larger `voxel`"):
        TF.fuse_tsdf_mesh(sc["depths"], sc["colors"], sc["K"], sc["R"], sc["t"], max_voxels=5000, device="cpu")
    with pytest.raises(ValueError, match=r"exceeds max_voxels"):
        TF.fuse_tsdf_mesh(sc["depths"], sc["colors"], sc["K"], sc["R"], sc["t"], voxel=1e-3, bounds=((0, 0, 0), (2, 2, 2)), device="cpu")
    with pytest.raises(ValueError, match="bounds"):
        TF.fuse_tsdf_mesh(sc["depths"], sc["colors"], sc["K"], sc["R"], sc["t"], bounds=((0, 0, 0), (2, -2, 2)), device="cpu")
    with pytest.raises(ValueError, match="voxel"):
        TF.fuse_tsdf_mesh(sc["depths"], sc["colors"], sc["K"], sc["R"], sc["t"], voxel=0.0, device="cpu")
    with pytest.raises(ValueError, match="no depth map has a valid pixel"):
        TF.fuse_tsdf_mesh([torch.zeros(4, 5)], [torch.zeros(4, 5, 3, dtype=torch.uint8)], sc["K"][:1], sc["R"][:1], sc["t"][:1], device="cpu")
    assert abs(TF.default_voxel(sc["depths"], sc["K"]) - 2 * 4.0 / 28.8) < 0.01
    assert TF.tsdf_options(Namespace()) == {}
    assert TF.tsdf_options(Namespace(tsdf_voxel=0.1, tsdf_trunc_voxels=4, tsdf_min_weight=2, tsdf_bounds=None)) == \
        dict(voxel=0.1, trunc_voxels=4, min_weight=2)


def test_run_writes_mesh_and_points(tmp_path, monkeypatch, capsys):
    """run(): the views of fusibile.masked_view go to fuse_tsdf_mesh with the options of args; the mesh lands under Meshes/, the
    vertices (tsdf_write_points) where the metrics mirror's read_ply finds them.  The three ops are replaced by the numpy rules; the grid is
    fuse_tsdf_mesh's own."""
    V, H, W, ds = 4, 24, 32, 2
    sc = synthetic.make_fusion_scene(V, H, W, exact=True)
    args = Namespace(model="mvsnet", nviews=V, data_path=str(tmp_path), scene="scan1", downscale=ds, colmap=False, filter=False,
                     prob_threshold=0.5, override=False, tsdf_trunc_voxels=3, tsdf_min_weight=1, tsdf_write_points=True)
    folder = f"{args.model}_{args.nviews}"
    dfold = tmp_path / "IntRes" / "depthmaps" / folder / "scan1"
    dfold.mkdir(parents=True)
    rng = np.random.default_rng(0)
    batches = []
    for v in range(V):
        name = f"{v:08d}"
        prob = np.ones((H, W), np.float32)
        if v == 0:
            prob[5:12, 8:20] = 0.2
        np.savez(dfold / f"{name}_out.npz", depthmap=sc["depths"][v].numpy(), probability=prob)
        order = [v] + [u for u in range(V) if u != v]
        Kf = sc["K"].clone()
        Kf[:, :2] *= ds
        batches.append({"filename": [name], "imgs": torch.from_numpy(rng.random((1, V, 3, H * ds, W * ds), dtype=np.float32)),
                        "K": Kf.unsqueeze(0)[:, order], "R": sc["R"].unsqueeze(0)[:, order], "t": sc["t"].unsqueeze(0)[:, order]})
    seen = {}

    def fake_integrate(state, depths, colors, cams, *, origin, voxel, trunc):
        seen.update(n=len(depths), masked=int((depths[0] == 0).sum()), trunc_voxels=round(trunc / voxel, 9), dims=state["weight"].shape[::-1])
        TR.integrate(state, [d.numpy() for d in depths], [c.numpy() for c in colors], cams.numpy(), origin, voxel, trunc)

    def fake_extract(state, *, origin, voxel, min_weight):
        seen.update(min_weight=min_weight)
        return tuple(torch.from_numpy(a) for a in TR.extract(state, origin, voxel, min_weight))

    monkeypatch.setattr(TF.ops, "tsdf_volume", lambda dims, device: TR.volume(dims))
    monkeypatch.setattr(TF.ops, "tsdf_integrate", fake_integrate)
    monkeypatch.setattr(TF.ops, "tsdf_extract", fake_extract)
    monkeypatch.setattr(TF, "fuse_tsdf_mesh", functools.partial(TF.fuse_tsdf_mesh, device="cpu"))
    TF.run(batches, args)
    assert seen == dict(trunc_voxels=3.0, min_weight=1, n=V, masked=7 * 12, dims=(25, 21, 10))
    out = tmp_path / "Meshes" / folder / f"{folder}scan1.ply"
    xyz, rgb, faces = PC.read_mesh(out)
    assert len(xyz) > 500 and len(faces) > 1000 and faces.max() == len(xyz) - 1
    cloud = PC.read_ply(tmp_path / "Points" / folder / f"{folder}scan1.ply")             # the reader of evaluation/metrics.py
    from wild_deep_mvs_amd.evaluation.metrics import format_point_cloud
    np.testing.assert_array_equal(format_point_cloud(cloud), xyz)
    np.testing.assert_array_equal(np.stack([cloud[c] for c in ("red", "green", "blue")], axis=1), rgb)
    stamp = out.read_bytes()
    out.write_bytes(b"stale")
    capsys.readouterr()
    TF.run(batches, args)
    assert "already computed" in capsys.readouterr().out and out.read_bytes() == b"stale"
    args.override = True
    TF.run(batches, args)
    assert out.read_bytes() == stamp
