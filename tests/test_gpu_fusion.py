"""GPU: depth-map fusion (pscv_fuse_depth_pass, csrc/depth_fusion.hip) against the float64 reference of tests/_fusion_bounds.py, its
determinism, a full-size identity property, the evaluation/fusibile.py run() mirror and the capacity check.

Each pass is compared on its own: the reference is handed the kernel's own used masks as they were before the pass, so an undecided
outcome of an earlier pass cannot cascade.  Decisions are thresholded fp32 quantities; each is evaluated over the interval its
derived rounding bound gives it, an undecided one widens the pixel's count range, and no pixel is exempt from anything."""
from argparse import Namespace

import numpy as np
import pytest
import torch

from tests import _fusion_cases as FC
from tests import _fusion_ref as FR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from wild_deep_mvs_amd import _lib as L, ops, synthetic
    from wild_deep_mvs_amd.evaluation import fusibile as EF
    L.lib()
    return L, ops, synthetic, EF


def _scene(synthetic, ops, V, H, W, seed=1, **kw):
    sc = synthetic.make_fusion_scene(V, H, W, seed=seed, **kw)
    cams = ops.geo_filter_cams(sc["K"], sc["R"], sc["t"])
    return sc, cams


@pytest.mark.parametrize("case,pname", [(c, p) for c in FC.SCENES for p in FC.PARAMS])
def test_each_pass_matches_the_rule(env, case, pname):
    """The four scenes (3 x 48x64, 9 x 48x64 ragged and behind, 33 x 40x56, 64 x 32x40) under both parameter pairs, through the
    shared comparison of tests/test_gpu_fusion_ref.py: every decided emit flag, positions within their propagated bound (and the
    flat 1e-5 bar, which that bound undercuts on every case), colours exactly, every mark placed."""
    L, ops, synthetic, EF = env
    from tests.test_gpu_fusion_ref import check_case
    V, H, W, kw = FC.SCENES[case]
    _, cams = _scene(synthetic, ops, V, H, W, **kw)
    np.testing.assert_array_equal(cams.numpy(), FC.get(f"{case}/{pname}")["cams"])      # the case's blocks are those of ops.geo_filter_cams
    stats = check_case(ops, f"{case}/{pname}")
    assert sum(s["points"] for s in stats) > 0 and sum(s["pos_checked"] for s in stats) > 1000


def test_fusion_is_deterministic(env):
    L, ops, synthetic, EF = env
    sc, cams = _scene(synthetic, ops, 9, 240, 320, half_res_view=4)
    args = ([d.cuda() for d in sc["depths"]], [c.cuda() for c in sc["colors"]], cams.cuda())
    a = ops.fuse_depth_maps(*args, disp_thresh=0.3, num_consistent=3)
    b = ops.fuse_depth_maps(*args, disp_thresh=0.3, num_consistent=3)
    assert a[0].shape[0] > 1000
    for x, y in zip(a, b):
        assert x.shape == y.shape and torch.equal(x, y)
    v = a[2].cpu().numpy()
    assert (np.diff(v) >= 0).all() and v[0] == 0           # pass-major


def test_full_size_identity(env):
    """49 copies of one camera and one depth map at 1200 x 1600: pass 0 emits exactly the valid pixels of view 0, each at its own
    unprojection (B = 0: every other view is consistent), and consumes everything; passes 1-48 emit nothing."""
    L, ops, synthetic, EF = env
    sc = synthetic.make_fusion_scene(1, 1200, 1600, seed=3)
    d0, c0 = sc["depths"][0], sc["colors"][0]
    V = 49
    cams = ops.geo_filter_cams(sc["K"].expand(V, 3, 3), sc["R"].expand(V, 3, 3), sc["t"].expand(V, 3, 1)).cuda()
    dg, cg = d0.cuda(), c0.cuda()
    xyz, rgb, view, pix = ops.fuse_depth_maps([dg] * V, [cg] * V, cams, disp_thresh=0.01, num_consistent=3, want_pixel=True)
    valid = np.flatnonzero(((d0 > 1e-3) & (d0 < 1e5)).numpy().reshape(-1))
    assert 0.95 * d0.numel() < valid.size < d0.numel()
    assert xyz.shape[0] == valid.size
    assert int(view.abs().max()) == 0
    np.testing.assert_array_equal(pix.cpu().numpy(), valid)
    K, Ki, R, t = FR.cam_parts(cams[:1].cpu().numpy())
    h, w = d0.shape
    ys, xs = np.divmod(valid, w)
    want = FR.unproject(Ki[0], R[0], t[0], xs.astype(np.float64), ys.astype(np.float64), d0.numpy().reshape(-1)[valid].astype(np.float64))
    got = xyz.cpu().numpy()
    err = np.abs(got - want).max(axis=1) / np.abs(want).max(axis=1)
    assert err.max() < 1e-5, err.max()
    np.testing.assert_array_equal(rgb.cpu().numpy(), c0.numpy().reshape(-1, 3)[valid])


def test_run_writes_the_upstream_file(env, tmp_path, capsys):
    """evaluation.fusibile.run: reads <scene>/<view>_out.npz depth + probability, masks like the reference (probability threshold,
    geo_mask of the geometric filter), colours like its gipuma images, fuses, writes Points/<model>_<nviews>/<model>_<nviews><scene>.ply."""
    L, ops, synthetic, EF = env
    V, H, W, ds = 5, 48, 64, 2
    sc, _ = _scene(synthetic, ops, V, H, W, seed=5)
    args = Namespace(model="mvsnet", nviews=V, data_path=str(tmp_path), scene="scan1", downscale=ds, colmap=False, filter=True,
                     prob_threshold=0.5, fusion_depth_threshold=0.3, fusion_num_consistent=2, override=False)
    folder = f"{args.model}_{args.nviews}"
    dfold = tmp_path / "IntRes" / "depthmaps" / folder / "scan1"
    gfold = tmp_path / "IntRes" / "geometric_filtering" / folder / "scan1"
    dfold.mkdir(parents=True)
    gfold.mkdir(parents=True)
    rng = np.random.default_rng(0)
    batches, masked, colors = [], [], []
    for v in range(V):
        name = f"{v:08d}"
        prob = np.ones((H, W), np.float32)
        geo = np.ones((H, W), bool)
        if v == 0:
            prob[10:30, 20:40] = 0.2                 # the known masked block of the reference view
        if v == 2:
            geo[:, :16] = False
        d = sc["depths"][v].numpy()
        np.savez(dfold / f"{name}_out.npz", depthmap=d, probability=prob)
        np.savez(gfold / f"{name}_out.npz", geo_mask=geo)
        img = torch.from_numpy(rng.random((1, V, 3, H * ds, W * ds), dtype=np.float32))
        Kf = sc["K"].clone()
        Kf[:, :2] *= ds
        batches.append({"filename": [name], "imgs": img, "K": Kf.unsqueeze(0)[:, [v] + [u for u in range(V) if u != v]],
                        "R": sc["R"].unsqueeze(0)[:, [v] + [u for u in range(V) if u != v]],
                        "t": sc["t"].unsqueeze(0)[:, [v] + [u for u in range(V) if u != v]]})
        dm = d.copy()
        dm[(prob < 0.5) | ~geo] = 0
        masked.append(dm)
        colors.append(EF.view_colors(img[0, 0], ds))
    assert colors[0].shape == (H, W, 3)
    EF.run(batches, args)
    out = tmp_path / "Points" / folder / f"{folder}scan1.ply"
    assert out.exists()
    data = FR.read_ply(out)
    xyz, rgb, view, pix = ops.fuse_depth_maps([torch.from_numpy(m).cuda() for m in masked], [torch.from_numpy(c).cuda() for c in colors],
                                              ops.geo_filter_cams(sc["K"], sc["R"], sc["t"]).cuda(), disp_thresh=0.3,
                                              num_consistent=2, want_pixel=True)
    assert len(data) == xyz.shape[0] > 1000
    np.testing.assert_array_equal(np.stack([data[c] for c in "xyz"], axis=1), xyz.cpu().numpy())
    np.testing.assert_array_equal(np.stack([data[c] for c in ("red", "green", "blue")], axis=1), rgb.cpu().numpy())
    v, p = view.cpu().numpy(), pix.cpu().numpy()
    ys, xs = np.divmod(p[v == 0], W)
    assert not ((ys >= 10) & (ys < 30) & (xs >= 20) & (xs < 40)).any(), "a point comes from a masked reference pixel"
    ys2, xs2 = np.divmod(p[v == 2], W)
    assert not (xs2 < 16).any()
    # second call: already computed, the file is left alone; override rewrites it
    stamp = out.read_bytes()
    out.write_bytes(b"stale")
    capsys.readouterr()
    EF.run(batches, args)
    assert "already computed" in capsys.readouterr().out and out.read_bytes() == b"stale"
    args.override = True
    EF.run(batches, args)
    assert out.read_bytes() == stamp


def test_capacity_overflow_is_a_clean_error(env):
    L, ops, synthetic, EF = env
    sc, cams = _scene(synthetic, ops, 5, 48, 64)
    args = ([d.cuda() for d in sc["depths"]], [c.cuda() for c in sc["colors"]], cams.cuda())
    full = ops.fuse_depth_maps(*args, disp_thresh=0.3, num_consistent=2)
    m = full[0].shape[0]
    assert m > 100
    with pytest.raises(L.PscvError, match="capacity"):
        ops.fuse_depth_maps(*args, disp_thresh=0.3, num_consistent=2, capacity=m - 1)
    with pytest.raises(L.PscvError, match="capacity"):
        used = [torch.zeros(d.shape, dtype=torch.uint8, device="cuda") for d in args[0]]
        ops.fuse_depth_pass(0, *args, used, disp_thresh=0.3, num_consistent=2, capacity=7)
    exact = ops.fuse_depth_maps(*args, disp_thresh=0.3, num_consistent=2, capacity=m)        # exactly enough
    torch.cuda.synchronize()
    for x, y in zip(full, exact):
        assert torch.equal(x, y)
    with pytest.raises(ValueError):
        ops.fuse_depth_maps(args[0], args[1][:-1], args[2])
