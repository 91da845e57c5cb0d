"""GPU: normal maps from depth maps (pscv_depth_normals, pscv_point_world_normals; csrc/depth_normals.hip) against the float64 rule
of tests/_depth_normals_ref.py, bit for bit; through ops.colmap_fuse; and behind the two fusion mirrors (args.fusion_normals).

The kernel's tile is 8 rows x 32 columns, so the parity shapes are 1 x 1, 5 x 7 (smaller than the r = 4 window), 9 x 33 (one past
a tile both ways), 37 x 45 (several tiles, ragged edges) and the 48 x 64 scene view, all in ONE call with radius 1, 2 and 4.

The fusion test states its 1 degree bar about a plane, so it is asserted where the fused surface is one:
``make_yfcc_fusion_scene(6, 48, 64)`` multiplies its plane's depths by 1 + 0.003 tanh(bump), and the true normal of that surface is
itself up to 2.7 degrees off the plane's (the float64 reference measures 2.0 to 2.7 degrees per view, per pixel, on it).  The
default scene carries every other assertion (same points with and without the normals, unit norms) and prints its angle (measured:
fused normals at most 1.69 degrees from the plane's); the bar is asserted on the same rig with ``perturb=0.0``, whose surface is the
plane (measured: 0.014 degrees)."""
from argparse import Namespace

import numpy as np
import pytest
import torch

from tests import _depth_normals_ref as DR

pytestmark = pytest.mark.gpu

RADII = (1, 2, 4)
MIN_SUPPORT = {1: 4, 2: 6, 4: 9}
GATE = 0.05


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from wild_deep_mvs_amd import _lib as L, ops, synthetic
    L.lib()
    return L, ops, synthetic


def _rotation(rng):
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    return q * np.sign(np.linalg.det(q))


def _cams(ops, shapes, rng):
    K = [[[0.9 * w + 3.0, 0.0, w / 2.0 + rng.uniform(-0.5, 0.5)], [0.0, 0.93 * w + 3.0, h / 2.0 + rng.uniform(-0.5, 0.5)],
          [0.0, 0.0, 1.0]] for h, w in shapes]
    R = np.stack([_rotation(rng) for _ in shapes])
    t = rng.standard_normal((len(shapes), 3, 1))
    return ops.geo_filter_cams(torch.tensor(K), torch.from_numpy(R), torch.from_numpy(t))


def _slanted(h, w, rng, base=3.0):
    """A slanted plane by its inverse depth, with a little fp32 noise: every window has a proper fit."""
    ys, xs = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    rho = 1.0 / base + 0.004 * xs / max(w, 2) - 0.003 * ys / max(h, 2)
    return ((1.0 / rho) * (1.0 + 1e-4 * rng.standard_normal((h, w)))).astype(np.float32)


@pytest.fixture(scope="module")
def views(env):
    """The depth maps of the parity test (different sizes, one call) and their cameras."""
    L, ops, synthetic = env
    rng = np.random.default_rng(11)
    one = np.full((1, 1), 2.0, dtype=np.float32)
    small = _slanted(5, 7, rng)
    step = _slanted(9, 33, rng)                       # a depth step below the gate, then one above it
    step[:, 12:20] *= np.float32(1.0 + 0.8 * GATE)
    step[:, 20:] *= np.float32(1.0 + 2.5 * GATE)
    holes = _slanted(37, 45, rng)
    holes[rng.random(holes.shape) < 0.08] = 0.0       # holes of zeros, a block of them, and every kind of invalid value
    holes[20:26, 30:41] = 0.0
    holes[3, 4], holes[8, 31], holes[33, 40] = np.nan, np.inf, -1.5
    holes[12:16, 5:9] *= np.float32(1.3)              # an island past the gate
    scene = synthetic.make_patch_match_scene(4, 48, 64, seed=3)["depth"][0].numpy().copy()
    dead = np.zeros((9, 33), dtype=np.float32)        # fully invalid
    dead[2, 3], dead[4, 30], dead[8, 32] = np.nan, -np.inf, -2.0
    row = np.zeros((10, 40), dtype=np.float32)        # the only valid pixels form one row: collinear, so every pixel falls back
    row[4] = _slanted(1, 40, rng)[0]
    maps = [one, small, step, holes, scene, dead, row]
    cams = _cams(ops, [m.shape for m in maps], rng)
    return maps, cams


_REF = {}


def _reference(views, r):
    """The rule's output for every parity view at radius r: computed once, shared, never written to."""
    if r not in _REF:
        maps, cams = views
        out = [DR.depth_normals(m, c, radius=r, rel_gate=GATE, min_support=MIN_SUPPORT[r]) for m, c in zip(maps, cams.numpy())]
        for n, s in out:
            n.setflags(write=False)
            s.setflags(write=False)
        _REF[r] = out
    return _REF[r]


def _ulps(a, b):
    """Distance in fp32 ulps between two finite float32 arrays (ordered-integer difference)."""
    key = lambda x: np.where(x.view(np.int32) < 0, np.int64(-2 ** 31) - x.view(np.int32).astype(np.int64), x.view(np.int32).astype(np.int64))
    return np.abs(key(a) - key(b))


@pytest.mark.parametrize("r", RADII)
def test_normals_and_supports_equal_the_rule(env, views, r):
    L, ops, synthetic = env
    maps, cams = views
    want = _reference(views, r)
    normals, supports = ops.depth_normals([torch.from_numpy(m).cuda() for m in maps], cams.cuda(), radius=r, rel_gate=GATE,
                                          min_support=MIN_SUPPORT[r], want_support=True)
    plain = ops.depth_normals([torch.from_numpy(m).cuda() for m in maps], cams.cuda(), radius=r, rel_gate=GATE,
                              min_support=MIN_SUPPORT[r])
    torch.cuda.synchronize()
    differ = total = fits = falls = 0
    for k, (m, (wn, ws)) in enumerate(zip(maps, want)):
        got_n, got_s = normals[k].cpu().numpy(), supports[k].cpu().numpy()
        assert got_n.shape == m.shape + (3,) and got_s.shape == m.shape
        np.testing.assert_array_equal(got_s, ws, err_msg=f"view {k} r={r}: support")
        assert torch.equal(plain[k], normals[k])                              # the same maps without the supports
        assert np.isfinite(got_n).all()
        u = _ulps(got_n, wn)
        assert u.max() <= 1, f"view {k} r={r}: a component is {u.max()} ulps from the rule"
        differ += int((u != 0).sum())
        total += u.size
        fits += int((ws > 0).sum())
        falls += int((ws < 0).sum())
    print(f"r={r}: {differ} of {total} components differ (by one ulp); {fits} fitted, {falls} fallback pixels")
    assert differ <= 1e-4 * total
    # the inputs do what they are there for
    assert fits > 3000 and falls > 40
    assert (want[5][1] == 0).all() and (want[5][0] == 0).all()                # the fully invalid map
    assert (want[6][1][4] < 0).all() and (np.delete(want[6][1], 4, axis=0) == 0).all()   # the one valid row: fallback
    assert want[0][1][0, 0] == -1                                             # 1 x 1: the centre alone
    s_step = want[2][1][4]
    full = (2 * r + 1) * min(2 * r + 1, 9)
    assert s_step[12] == full and s_step[20] == s_step[19] < full             # the step below the gate joins, the one above splits


def test_65_views_in_one_call_equal_65_calls(env):
    L, ops, synthetic = env
    rng = np.random.default_rng(5)
    V = L.FUSE_MAX_VIEWS + 1
    maps = [torch.from_numpy(_slanted(5, 7, rng, base=2.0 + 0.05 * v)).cuda() for v in range(V)]
    maps[7][2, 3] = 0.0
    cams = _cams(ops, [(5, 7)] * V, rng).cuda()
    normals, supports = ops.depth_normals(maps, cams, want_support=True)
    assert len(normals) == len(supports) == V
    for v in range(V):
        n1, s1 = ops.depth_normals(maps[v:v + 1], cams[v:v + 1], want_support=True)
        assert torch.equal(n1[0], normals[v]) and torch.equal(s1[0], supports[v]), f"view {v}"
    assert not torch.equal(normals[0], normals[64])
    want_n, want_s = DR.depth_normals(maps[64].cpu().numpy(), cams[64].cpu().numpy())      # the view past the chunk, against the rule
    np.testing.assert_array_equal(supports[64].cpu().numpy(), want_s)
    assert _ulps(normals[64].cpu().numpy(), want_n).max() <= 1


def test_point_world_normals_equal_the_rule(env):
    L, ops, synthetic = env
    rng = np.random.default_rng(9)
    shapes = [(5, 7), (37, 45), (9, 33)]
    cams = _cams(ops, shapes, rng)
    normals = [rng.standard_normal(s + (3,)).astype(np.float32) for s in shapes]
    M = 1000
    view = rng.integers(0, 3, M).astype(np.int32)
    pixel = np.array([rng.integers(0, shapes[v][0] * shapes[v][1]) for v in view], dtype=np.int32)
    for k, v in enumerate((0, 1, 2)):                                         # the last pixel of every view is among them
        view[k], pixel[k] = v, shapes[v][0] * shapes[v][1] - 1
    view[10] = 3                                                              # indices outside their range: (0, 0, 0), nothing is read
    view[11], pixel[11] = 0, 5 * 7
    pixel[12], view[13] = -1, -1
    want = DR.point_world_normals(view, pixel, normals, cams.numpy())
    got = ops.point_world_normals(torch.from_numpy(view).cuda(), torch.from_numpy(pixel).cuda(), [torch.from_numpy(n).cuda() for n in normals],
                                  cams.cuda())
    torch.cuda.synchronize()
    np.testing.assert_array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert (want[[10, 11, 12, 13]] == 0).all() and np.abs(want).sum() > 100
    empty = ops.point_world_normals(torch.zeros(0, dtype=torch.int32, device="cuda"), torch.zeros(0, dtype=torch.int32, device="cuda"),
                                    [torch.from_numpy(n).cuda() for n in normals], cams.cuda())
    assert tuple(empty.shape) == (0, 3)


def _fusion_inputs(ops, sc):
    cams = ops.geo_filter_cams(sc["K"], sc["R"], sc["t"]).cuda()
    return [d.cuda() for d in sc["depths"]], [c.cuda() for c in sc["colors"]], cams


PLANE_NORMAL = np.array([0.10, -0.06, 1.0]) / np.linalg.norm([0.10, -0.06, 1.0])      # of make_yfcc_fusion_scene; the cameras see -n


@pytest.mark.parametrize("perturb", [None, 0.0], ids=["default", "plane"])
def test_fusion_with_depth_normals_keeps_the_points(env, perturb):
    L, ops, synthetic = env
    sc = synthetic.make_yfcc_fusion_scene(6, 48, 64, **({} if perturb is None else {"perturb": perturb}))
    depths, colors, cams = _fusion_inputs(ops, sc)
    normals = ops.depth_normals(depths, cams)
    # precondition on the inputs: no two world normals are near opposite (at 180 degrees the test is w_s . w_p >= -1 on fp32 vectors)
    idx = [torch.nonzero(d.reshape(-1) > 0).reshape(-1).to(torch.int32) for d in depths]
    W = torch.cat([ops.point_world_normals(torch.full_like(p, v), p, normals, cams) for v, p in enumerate(idx)])
    lowest = min(float((W[k:k + 2048] @ W.T).min()) for k in range(0, W.shape[0], 2048))
    assert W.shape[0] > 10000 and lowest >= -0.5, lowest
    kw = dict(max_depth_error=0.01, max_reproj_error=1.0, min_num_pixels=3)
    xyz0, nor0, rgb0, view0 = ops.colmap_fuse(depths, colors, cams, sc["overlap"], **kw)
    xyz, nor, rgb, view = ops.colmap_fuse(depths, colors, cams, sc["overlap"], normals=normals, max_normal_error=180.0, **kw)
    torch.cuda.synchronize()
    assert xyz.shape[0] > 1000
    assert torch.equal(xyz.view(torch.int32), xyz0.view(torch.int32)) and torch.equal(rgb, rgb0) and torch.equal(view, view0)
    n = nor.cpu().numpy().astype(np.float64)
    assert np.abs(np.linalg.norm(n, axis=1) - 1.0).max() <= 1e-6
    ang = np.degrees(np.arccos(np.clip(-(n @ PLANE_NORMAL), -1.0, 1.0)))
    print(f"perturb={perturb}: {xyz.shape[0]} points, fused normals at most {ang.max():.4f} degrees from the plane's, lowest dot {lowest:.3f}")
    assert not torch.equal(nor, nor0)
    if perturb == 0.0:
        assert ang.max() <= 1.0


def test_normal_test_refuses_a_tilted_slab(env):
    """make_normal_fusion_scene's view 1 with its central block replaced by a slab hinged on the true plane along one of the
    block's columns (the one with the most plane around it) and tilted about it.  Near the hinge the slab's depths still pass the fusion's depth test, so at 180 degrees
    seeds of the other views take slab pixels; at 10 degrees the slab's estimated normals refuse every one of them.  Slab pixels
    whose window also holds pixels outside the slab have mixed normals and are left out (the interior: r = 2 from its border)."""
    L, ops, synthetic = env
    V, H, W, rot = 4, 48, 64, 1
    sc = synthetic.make_normal_fusion_scene(V, H, W, seed=3)
    block = sc["rotated"][rot].numpy()
    ys, xs = np.nonzero(block)
    y0, y1, x0, x1 = ys.min(), ys.max() + 1, xs.min(), xs.max() + 1
    gt = sc["depth_gt"][rot].numpy().astype(np.float64)
    plane = gt > 4.0                                                          # (the sphere is nearer than 3.6, the plane about 5)
    gy, gx = np.nonzero(plane)
    coef = np.linalg.lstsq(np.stack((gx, gy, np.ones_like(gx)), axis=1).astype(np.float64), 1.0 / gt[plane], rcond=None)[0]
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    rho = coef[0] * xx + coef[1] * yy + coef[2]                               # the plane's inverse depth: affine in the pixel
    assert np.abs(rho[plane] * gt[plane] - 1.0).max() < 1e-6
    hinge = max(range(x0 + 3, x1 - 3), key=lambda x: int(plane[y0 + 2:y1 - 2, x - 1:x + 2].sum()))     # where view 1 sees the plane itself
    slab = 1.0 / (rho + 0.0016 * (xx - hinge))                                # another plane through the hinge column
    d = sc["depths"][rot].numpy().copy()
    put = block & (d > 0)
    d[put] = slab[put].astype(np.float32)
    depths = [x.clone() for x in sc["depths"]]
    depths[rot] = torch.from_numpy(d)
    depths = [x.cuda() for x in depths]
    colors = [c.cuda() for c in sc["colors"]]
    cams = ops.geo_filter_cams(sc["K"], sc["R"], sc["t"]).cuda()
    normals = ops.depth_normals(depths, cams)
    interior = np.zeros((H, W), dtype=bool)
    interior[y0 + 2:y1 - 2, x0 + 2:x1 - 2] = True
    # precondition: inside the slab the estimated normal is far more than 10 degrees from the plane's
    wn = DR.world_normal(cams[rot].cpu().numpy(), normals[rot].cpu().numpy()).astype(np.float64)
    true_w = sc["normal_world"][rot].numpy().astype(np.float64)[plane][0]
    sel = interior & put & (ops.depth_normals(depths, cams, want_support=True)[1][rot].cpu().numpy() == 25)
    tilt = np.degrees(np.arccos(np.clip(wn[sel] @ true_w, -1.0, 1.0)))
    assert sel.sum() > 100 and tilt.min() > 20.0, (sel.sum(), tilt.min())
    kw = dict(max_depth_error=0.01, max_reproj_error=1.0, min_num_pixels=3)
    joined = {}
    for err in (180.0, 10.0):
        joined[err] = 0
        for u in range(V):
            if u == rot:
                continue
            fused = [torch.zeros(x.shape, dtype=torch.uint8, device="cuda") for x in depths]
            ops.colmap_fuse_pass(u, depths, colors, cams, sc["overlap"], fused, normals=normals, max_normal_error=err, **kw)
            joined[err] += int(fused[rot].cpu().numpy()[interior & put].sum())
    print(f"slab of {sel.sum()} interior pixels tilted {tilt.min():.1f}-{tilt.max():.1f} degrees: {joined[180.0]} joins at 180 degrees, "
          f"{joined[10.0]} at 10")
    assert joined[180.0] >= 10 and joined[10.0] == 0


# ---- the mirrors ------------------------------------------------------------------------------------------------------------------
def _ply(path):
    from wild_deep_mvs_amd.utils.point_cloud import read_ply
    data = read_ply(path)
    cols = lambda names: np.stack([data[c] for c in names], axis=1)
    return data, cols("xyz"), cols(("red", "green", "blue"))


def test_colmap_fusion_mirror_with_depth_normals(env, tmp_path):
    L, ops, synthetic = env
    from wild_deep_mvs_amd.evaluation import colmap_fusion as CF, metrics as M
    V, H, W, ds = 5, 24, 32, 2
    sc = synthetic.make_yfcc_fusion_scene(V, H, W, seed=4)
    args = Namespace(model="vis", nviews=V, data_path=str(tmp_path), scene="sceneA_5", downscale=ds, colmap=False, filter=True,
                     upsample=False, prob_threshold=0.5, fusion_depth_threshold=0.01, fusion_max_reproj_error=1.0,
                     fusion_num_consistent=3, override=True, dataset="yfcc")
    folder = f"{args.model}_{args.nviews}"
    dfold = tmp_path / "IntRes" / "depthmaps" / folder / "sceneA_5"
    gfold = tmp_path / "IntRes" / "geometric_filtering" / folder / "sceneA_5"
    dfold.mkdir(parents=True)
    gfold.mkdir(parents=True)
    rng = np.random.default_rng(0)
    batches, masked = [], []
    for v in range(V):
        name = f"{v:08d}"
        d = sc["depths"][v].numpy()
        h, w = d.shape
        prob = np.ones((h, w), np.float32)
        prob[2:6, 3:9] = 0.2
        geo = np.ones((h, w), bool)
        geo[:, :2] = False
        np.savez(dfold / f"{name}_out.npz", depthmap=d, probability=prob)
        np.savez(gfold / f"{name}_out.npz", geo_mask=geo)
        img = torch.from_numpy(rng.random((1, 1, 3, h * ds, w * ds), dtype=np.float32))
        Kf = sc["K"][v].clone().double()
        Kf[:2] *= ds
        batches.append({"filename": [name], "imgs": img, "K": Kf.float()[None, None], "R": sc["R"][v][None, None],
                        "t": sc["t"][v][None, None]})
        dm = d.copy()
        dm[(prob < 0.5) | ~geo] = 0
        masked.append(dm)
    out = tmp_path / "Points" / folder / f"{folder}sceneA_5.ply"
    CF.colmap_fusion(batches, args)
    default_bytes = out.read_bytes()
    data0, xyz0, rgb0 = _ply(out)
    CF.colmap_fusion(batches, Namespace(**vars(args), fusion_normals="constant"))
    assert out.read_bytes() == default_bytes                                  # "constant" is the default path
    CF.colmap_fusion(batches, Namespace(**vars(args), fusion_normals="depth", fusion_normal_radius=1, fusion_normal_support=4))
    data, xyz, rgb = _ply(out)
    assert len(data) == len(data0) > 100
    np.testing.assert_array_equal(xyz.view(np.uint32), xyz0.view(np.uint32))
    np.testing.assert_array_equal(rgb, rgb0)
    nor0, nor = (np.stack([dd[c] for c in ("nx", "ny", "nz")], axis=1) for dd in (data0, data))
    assert not np.array_equal(nor, nor0)                                      # not the medians of the views' constant normals
    assert len(np.unique(nor.round(5), axis=0)) > 50 and np.abs(np.linalg.norm(nor.astype(np.float64), axis=1) - 1.0).max() <= 1e-6
    # they are the normals of the maps the fusion read, at the options the arguments name
    K = sc["K"].clone().double()
    K[:, :2] = (K[:, :2] * ds) / ds
    cams = ops.geo_filter_cams(K.float(), sc["R"], sc["t"]).cuda()
    dm = [torch.from_numpy(m).cuda() for m in masked]
    want = ops.colmap_fuse(dm, [torch.from_numpy(CF.nearest_colors(b["imgs"][0, 0], *m.shape)).cuda() for b, m in zip(batches, masked)],
                           cams, [[u for u in range(V) if u != v] for v in range(V)], max_depth_error=0.01, max_reproj_error=1.0,
                           min_num_pixels=3, normals=ops.depth_normals(dm, cams, radius=1, min_support=4), max_normal_error=180.0)
    np.testing.assert_array_equal(nor.view(np.uint32), want[1].cpu().numpy().view(np.uint32))
    np.testing.assert_array_equal(M.format_point_cloud(data), xyz0)           # what metrics.run reads from the file


def test_fusibile_mirror_with_depth_normals(env, tmp_path):
    L, ops, synthetic = env
    from wild_deep_mvs_amd.evaluation import fusibile as EF, metrics as M
    V, H, W, ds = 5, 48, 64, 2
    sc = synthetic.make_fusion_scene(V, H, W, seed=5)
    args = Namespace(model="mvsnet", nviews=V, data_path=str(tmp_path), scene="scan1", downscale=ds, colmap=False, filter=False,
                     prob_threshold=0.5, fusion_depth_threshold=0.3, fusion_num_consistent=2, override=True)
    folder = f"{args.model}_{args.nviews}"
    dfold = tmp_path / "IntRes" / "depthmaps" / folder / "scan1"
    dfold.mkdir(parents=True)
    rng = np.random.default_rng(0)
    batches, masked, colors = [], [], []
    order = lambda v: [v] + [u for u in range(V) if u != v]
    Kf = sc["K"].clone()
    Kf[:, :2] *= ds
    for v in range(V):
        name = f"{v:08d}"
        prob = np.ones((H, W), np.float32)
        prob[10:30, 20 + v:40 + v] = 0.2
        d = sc["depths"][v].numpy()
        np.savez(dfold / f"{name}_out.npz", depthmap=d, probability=prob)
        img = torch.from_numpy(rng.random((1, V, 3, H * ds, W * ds), dtype=np.float32))
        batches.append({"filename": [name], "imgs": img, "K": Kf.unsqueeze(0)[:, order(v)], "R": sc["R"].unsqueeze(0)[:, order(v)],
                        "t": sc["t"].unsqueeze(0)[:, order(v)]})
        dm = d.copy()
        dm[prob < 0.5] = 0
        masked.append(torch.from_numpy(dm).cuda())
        colors.append(torch.from_numpy(EF.view_colors(img[0, 0], ds)).cuda())
    out = tmp_path / "Points" / folder / f"{folder}scan1.ply"
    EF.run(batches, args)
    default_bytes = out.read_bytes()
    data0, xyz0, rgb0 = _ply(out)
    assert data0.dtype.names == ("x", "y", "z", "red", "green", "blue")       # the plain layout, as before
    EF.run(batches, Namespace(**vars(args), fusion_normals="constant"))
    assert out.read_bytes() == default_bytes
    EF.run(batches, Namespace(**vars(args), fusion_normals="depth"))
    data, xyz, rgb = _ply(out)
    assert data.dtype.names == ("x", "y", "z", "nx", "ny", "nz", "red", "green", "blue")
    assert len(data) == len(data0) > 1000
    np.testing.assert_array_equal(xyz.view(np.uint32), xyz0.view(np.uint32))
    np.testing.assert_array_equal(rgb, rgb0)
    cams = ops.geo_filter_cams(sc["K"], sc["R"], sc["t"]).cuda()
    _, _, view, pixel = ops.fuse_depth_maps(masked, colors, cams, disp_thresh=0.3, num_consistent=2, want_pixel=True)
    want = ops.point_world_normals(view, pixel, ops.depth_normals(masked, cams), cams).cpu().numpy()
    nor = np.stack([data[c] for c in ("nx", "ny", "nz")], axis=1)
    np.testing.assert_array_equal(nor.view(np.uint32), want.view(np.uint32))
    assert np.abs(np.linalg.norm(nor.astype(np.float64), axis=1) - 1.0).max() <= 1e-6 and len(np.unique(nor.round(4), axis=0)) > 50
    np.testing.assert_array_equal(M.format_point_cloud(data), xyz0)           # what metrics.run reads from the file
