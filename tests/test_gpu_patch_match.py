"""GPU: PatchMatch stereo (csrc/patch_match.hip) against the numpy rule of tests/_patch_match_ref.py.
Costs to 1e-4 with exact invalid flags (grazing planes to their derived bound); half-steps with identical candidates, the same
choice wherever the oracle's best two costs are 1e-3 apart and a regret inside the derived bounds at every pixel; determinism; the
accuracy bars on make_patch_match_scene after the geometric pass and the filter; the geometric pass's gain; the filter against
the oracle, every pixel's count inside its decided range; the evaluation/colmap_stereo.py mirror; every limit.  The per-entry
checks with derived bounds at every shape, window and source count are in tests/test_gpu_patch_match_ref.py."""
import math
from argparse import Namespace

import numpy as np
import pytest
import torch

from tests import _patch_match_bounds as PB
from tests import _patch_match_ref as PR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from wild_deep_mvs_amd import _lib as L, ops, synthetic
    L.lib()
    return L, ops, synthetic


def _scene(synthetic, ops, V, H, W, seed=0):
    sc = synthetic.make_patch_match_scene(V, H, W, seed=seed)
    greys = [PR.grey(sc["imgs"][v].numpy()) for v in range(V)]
    cams = ops.geo_filter_cams(sc["K"], sc["R"], sc["t"])
    return sc, greys, cams


def _random_state(rng, h, w, Kinv, dmin, dmax):
    rows, cols = np.divmod(np.arange(h * w), w)
    m = np.stack([cols, rows, np.ones(h * w)], -1) @ Kinv.T
    n = rng.standard_normal((h * w, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    n = np.where(((n * m).sum(1) > 0)[:, None], -n, n)
    d = 1.0 / rng.uniform(1.0 / dmax, 1.0 / dmin, h * w)
    return np.concatenate([d[:, None], n], 1).reshape(h, w, 4).astype(np.float32)


def _look(c, target):
    z = np.asarray(target, float) - c
    z /= np.linalg.norm(z)
    x = np.cross([0.0, 1.0, 0.0], z)
    x /= np.linalg.norm(x)
    R = np.stack([x, np.cross(z, x), z])
    return R, -R @ c


def test_cost_matches_oracle_with_every_invalid_class(env):
    L, ops, synthetic = env
    sc, greys, cams = _scene(synthetic, ops, 3, 40, 56)
    ref = greys[0].copy()
    ref[4:20, 4:20] = 0.5                                    # low reference variance
    K0, R0, t0 = sc["K"][0].double().numpy(), sc["R"][0].double().numpy(), sc["t"][0].double().numpy()
    c0 = -R0.T @ t0[:, 0]
    Ks, Rs, ts, imgs = [sc["K"][1], sc["K"][2]], [sc["R"][1], sc["R"][2]], [sc["t"][1], sc["t"][2]], [greys[1], greys[2]]
    extra = [(c0 - 0.5 * R0[2], c0 - 10.0 * R0[2]),                                    # looking away: the scene is behind it
             (c0 + np.array([0.004, 0.0, 0.0]), c0 + R0[2] * 4.5),                      # 1 mm-ish baseline: angle < 1 deg
             (c0 + np.array([0.3, 0.0, 0.0]), c0 + R0[2] * 4.5 + np.array([2.5, 0.0, 0.0]))]   # turned: part outside
    for k, (c, tgt) in enumerate(extra):
        R, t = _look(c, tgt)
        Ks.append(sc["K"][0]); Rs.append(torch.from_numpy(R).float()); ts.append(torch.from_numpy(t.reshape(3, 1)).float())
        imgs.append(greys[1 + k % 2])
    cams_np = ops.geo_filter_cams(torch.stack([sc["K"][0]] + Ks), torch.stack([sc["R"][0]] + Rs), torch.stack([sc["t"][0]] + ts))
    h, w = ref.shape
    rng = np.random.default_rng(3)
    state = _random_state(rng, h, w, np.linalg.inv(K0), float(sc["depth_min"][0]), float(sc["depth_max"][0]))
    cost, err, agg = ops.patch_match_cost(torch.from_numpy(state).cuda(), torch.from_numpy(ref).cuda(),
                                          [torch.from_numpy(g).cuda() for g in imgs], cams_np.cuda())
    assert err is None
    rows, cols = np.divmod(np.arange(h * w), w)
    oc, vr, vs, _ = PR.source_costs(ref, imgs, cams_np.numpy(), rows, cols, state[..., 0].reshape(-1), state[..., 1:].reshape(-1, 3))
    kc = cost.cpu().numpy().reshape(len(imgs), -1)
    near = (np.abs(vr - PR.MIN_VAR) < 0.01 * PR.MIN_VAR)[None] | (np.abs(vs - PR.MIN_VAR) < 0.01 * PR.MIN_VAR)
    inv_o, inv_k = oc == 2.0, kc == 2.0
    assert np.array_equal(inv_o[~near], inv_k[~near])
    # fp32 homographies lose precision on planes seen within ~6 deg of grazing (|cos| of normal and ray < 0.1): the taps' positions
    # cancel there; the flat 1e-4 bar holds away from them, and they are held to their own derived bound below
    ray = np.stack([cols, rows, np.ones(h * w)], -1) @ np.linalg.inv(K0).T
    cosv = np.abs((state[..., 1:].reshape(-1, 3) * ray).sum(1)) / np.linalg.norm(ray, axis=1)
    ok = ~near & ~inv_o & (cosv >= 0.1)[None]
    dc = np.abs(kc - oc)
    worst = np.unravel_index(np.argmax(np.where(~near & ~inv_o, dc, 0)), dc.shape)
    print(f"\n[patch_match] cost: max |dc| {dc[~near & ~inv_o].max():.2e} at source {worst[0]} (|cos| {cosv[worst[1]]:.3f}, "
          f"var_r {vr[worst[1]]:.2e}, var_s {vs[worst]:.2e}); {dc[ok].max():.2e} away from grazing planes, {ok.sum()} entries")
    assert dc[ok].max() <= 1e-4
    cm = PB.cost_model(ref, imgs, cams_np.numpy(), rows, cols, state[..., 0].reshape(-1), state[..., 1:].reshape(-1, 3))
    graz = cm["vdec"] & cm["valid"] & (cosv < 0.1)[None]
    print(f"[patch_match] grazing planes: {graz.sum()} entries, worst |dc| / bound {(dc[graz] / (cm['cb'][graz] * PB.SCALE['cost'])).max():.3f}")
    assert graz.sum() > 100 and (dc[graz] <= cm["cb"][graz] * PB.SCALE["cost"]).all()
    dec = cm["vdec"]
    assert np.array_equal(inv_k[dec], ~cm["valid"][dec])              # no band: every decided flag, the variance tests included
    # every invalid class occurs
    assert inv_o[2].all() and inv_o[3].mean() > 0.99             # behind; angle < 1 deg
    assert 0.05 < inv_o[4].mean() < 0.95                          # partly outside
    lowvar = (rows >= 9) & (rows < 15) & (cols >= 9) & (cols < 15)
    assert inv_o[:, lowvar].all() and (vr[lowvar] < PR.MIN_VAR).all()
    assert np.abs(agg.cpu().numpy().reshape(-1) - PR.aggregate(oc, 3))[~near.any(0) & (cosv >= 0.1)].max() <= 1e-4


@pytest.mark.parametrize("S", [1, 4, 9, 19])
@pytest.mark.parametrize("geometric", [False, True])
def test_half_step_matches_oracle(env, S, geometric):
    L, ops, synthetic = env
    sc, greys, cams = _scene(synthetic, ops, 20, 24, 32, seed=1)
    src = sc["src"][0][:S]
    cams_v = cams[[0] + src].contiguous()
    h, w = greys[0].shape
    dmin, dmax = float(sc["depth_min"][0]), float(sc["depth_max"][0])
    st0 = ops.patch_match_init(h, w, cams_v.cuda(), dmin, dmax, seed=5, view=7)
    init_o = PR.init_state(h, w, cams_v.numpy(), dmin, dmax, 5, 7)
    init_v, init_b, init_dec = PB.init_model(h, w, cams_v.numpy(), dmin, dmax, 5, 7)
    assert np.abs(init_v - init_o).max() <= 1e-9
    assert (np.abs(st0.cpu().numpy() - init_v) <= init_b * PB.SCALE["init"])[init_dec].all()      # per element, derived
    # start from a half-converged state: ground truth on the left half, the random initialisation on the right
    state = st0.cpu().numpy()
    gt = np.concatenate([sc["depth"][0].numpy()[..., None], sc["normal"][0].numpy()], -1)
    state[:, : w // 2] = gt[:, : w // 2]
    sd = [torch.from_numpy(sc["depth"][s].numpy() * np.float32(1.003)).cuda() for s in src] if geometric else None
    ref = torch.from_numpy(greys[0]).cuda()
    srcs = [torch.from_numpy(greys[s]).cuda() for s in src]
    for colour in (0, 1):
        it = (int(geometric) << 16) | 2
        delta, theta = ops.patch_match_schedule(2)
        st = torch.from_numpy(state).cuda()
        choice, cand = ops.patch_match_half_step(st, ref, srcs, cams_v.cuda(), dmin, dmax, colour=colour, iteration=it, delta=delta,
                                                 theta=theta, seed=5, view=7, src_depths=sd, want_choice=True, want_candidates=True)
        new_o, ch_o, cd_o, gap, amb = PR.half_step(state, greys[0], [greys[s] for s in src], cams_v.numpy(), dmin, dmax,
                                                   colour=colour, iteration=it, delta=delta, theta=theta, seed=5, view=7,
                                                   src_depths=None if sd is None else [d.cpu().numpy() for d in sd])
        cd_k = cand.cpu().numpy()
        mine = ((np.add.outer(np.arange(h), np.arange(w)) & 1) == colour)
        skip_o, skip_k = (cd_o[mine] == 0).all(-1), (cd_k[mine] == 0).all(-1)
        assert np.array_equal(skip_o, skip_k)
        a, b = cd_o[mine][~skip_o], cd_k[mine][~skip_o]
        assert np.abs(a[:, 0] - b[:, 0]).max() <= 1e-4 * np.abs(a[:, 0]).max()
        assert np.abs(a[:, 1:] - b[:, 1:]).max() <= 1e-4
        ch_k = choice.cpu().numpy()
        assert (ch_k[~mine] == -1).all()
        sure = mine & (gap > 1e-3) & ~amb
        assert np.array_equal(ch_k[sure], ch_o[sure])
        # every pixel of the colour, sure or not: the chosen candidate's float64 cost is within the two bounds of the minimum, and
        # among bit-identical candidates the lowest index was chosen
        case = Namespace(ref=greys[0], srcs=[greys[s] for s in src], cams=cams_v.numpy(), radius=5, step=1, top_k=min(S, 3), h=h, w=w,
                         sdepths=None if sd is None else [d.cpu().numpy() for d in sd])
        from tests import _patch_match_cases as CS
        res, _ = PB.check_choice(cd_k[mine], ch_k[mine], CS.agg_of(case, geometric, colour))
        print(PB.fmt(f"S={S} geometric={geometric} colour={colour}", res))
        assert not PB.failures(res), res
        # the written state is the chosen candidate
        ks = st.cpu().numpy()
        pick = np.take_along_axis(cd_k, np.clip(ch_k, 0, 10)[..., None, None], axis=2)[:, :, 0]
        assert np.array_equal(ks[mine], pick[mine]) and np.array_equal(ks[~mine], state[~mine])


def _reconstruct(ops, sc, greys, cams, iters=8):
    V = len(greys)
    g = [torch.from_numpy(x).cuda() for x in greys]
    photo, geom, depth, normal, counts = [], [], [], [], []
    for v in range(V):
        ids = [v] + sc["src"][v]
        photo.append(ops.patch_match(g[v], [g[s] for s in sc["src"][v]], cams[ids].cuda(), float(sc["depth_min"][v]),
                                     float(sc["depth_max"][v]), num_iterations=iters, view=v))
    for v in range(V):
        ids = [v] + sc["src"][v]
        sd = [photo[s][..., 0].contiguous() for s in sc["src"][v]]
        st = ops.patch_match(g[v], [g[s] for s in sc["src"][v]], cams[ids].cuda(), float(sc["depth_min"][v]), float(sc["depth_max"][v]),
                             num_iterations=iters, view=v, src_depths=sd, state=photo[v])
        d, n, c = ops.patch_match_filter(st, g[v], [g[s] for s in sc["src"][v]], cams[ids].cuda(), sd, want_count=True)
        geom.append(st); depth.append(d.cpu().numpy()); normal.append(n.cpu().numpy()); counts.append(c)
    return photo, geom, depth, normal, counts


def test_determinism(env):
    L, ops, synthetic = env
    sc, greys, cams = _scene(synthetic, ops, 4, 48, 64)
    a = _reconstruct(ops, sc, greys, cams, iters=3)
    b = _reconstruct(ops, sc, greys, cams, iters=3)
    for x, y in zip(a[0] + a[1], b[0] + b[1]):
        assert torch.equal(x, y)
    for x, y in zip(a[2], b[2]):
        assert np.array_equal(x, y)


# The within-1 % bar is 0.90 at 192 x 256.  At 96 x 128 it is 0.80: there 1 % of depth is about 0.1 px of disparity for the
# median baseline, below what an 11 x 11 NCC resolves on this texture (measured 0.83; 0.95 at 192 x 256).
@pytest.mark.parametrize("V,H,W,within_bar", [(5, 96, 128, 0.80), (10, 192, 256, 0.90)])
def test_accuracy_geometric_pass_and_filter(env, V, H, W, within_bar):
    L, ops, synthetic = env
    sc, greys, cams = _scene(synthetic, ops, V, H, W)
    photo, geom, depth, normal, _ = _reconstruct(ops, sc, greys, cams)
    within, kept, nerr, untex = PR.accuracy(depth, normal, sc["depth"].numpy(), sc["normal"].numpy(), sc["untextured"].numpy(),
                                            sc["vis"].numpy())
    print(f"\n[patch_match] {V} views {H}x{W}: within 1% {within:.3f}, kept {kept:.3f}, median normal error {nerr:.2f} deg, "
          f"untextured filtered {untex:.3f}")
    assert within >= within_bar and kept >= 0.70 and nerr <= 10.0 and untex >= 0.90
    # the geometric pass raises the fraction of pixels with e_s <= 1 px in >= 2 sources
    g = [torch.from_numpy(x).cuda() for x in greys]
    frac = []
    for states in (photo, geom):
        n_ok = 0
        for v in range(V):
            ids = [v] + sc["src"][v]
            sd = [photo[s][..., 0].contiguous() for s in sc["src"][v]]
            _, err, _ = ops.patch_match_cost(states[v], g[v], [g[s] for s in sc["src"][v]], cams[ids].cuda(), src_depths=sd)
            n_ok += int(((err <= 1.0).sum(0) >= 2).sum())
        frac.append(n_ok / (V * H * W))
    print(f"[patch_match] e_s <= 1 px in >= 2 sources: photometric {frac[0]:.3f}, geometric {frac[1]:.3f}")
    assert frac[1] > frac[0]


def test_filter_matches_oracle(env):
    L, ops, synthetic = env
    sc, greys, cams = _scene(synthetic, ops, 4, 48, 64, seed=2)
    photo, geom, depth, normal, counts = _reconstruct(ops, sc, greys, cams, iters=4)
    for v in range(4):
        src = sc["src"][v]
        ids = [v] + src
        cnt_o, margin = PR.filter_counts(geom[v].cpu().numpy(), greys[v], [greys[s] for s in src], cams[ids].numpy(),
                                         [photo[s][..., 0].cpu().numpy() for s in src])
        keep_o = cnt_o >= PR.FILTER_MIN_CONSISTENT
        keep_k = depth[v] > 0
        fm = PB.filter_model(geom[v].cpu().numpy(), greys[v], [greys[s] for s in src], cams[ids].numpy(),
                             [photo[s][..., 0].cpu().numpy() for s in src])
        res = PB.check_filter(fm, geom[v].cpu().numpy(), depth[v], normal[v], counts[v].cpu().numpy())
        assert not PB.failures(res), res                        # every pixel: the count inside its decided range
        assert np.array_equal(keep_o[~margin], keep_k[~margin])
        assert np.array_equal(counts[v].cpu().numpy()[~margin], cnt_o[~margin])
        st = geom[v].cpu().numpy()
        assert np.array_equal(depth[v][keep_k], st[..., 0][keep_k]) and (normal[v][~keep_k] == 0).all()


def test_depthmap_colmap_mirror(env, tmp_path):
    L, ops, synthetic = env
    from wild_deep_mvs_amd.evaluation.colmap_stereo import depthmap_colmap
    from wild_deep_mvs_amd.utils.colmap_array import read_array
    sc = synthetic.make_patch_match_scene(4, 48, 64, seed=3)
    batches = synthetic.patch_match_batches(sc)
    args = Namespace(data_path=str(tmp_path), scene="s0", pm_iterations=3)
    depthmap_colmap(batches, args)
    stereo = tmp_path / "IntRes" / "colmap_dense" / "s0" / "stereo"
    for b in batches:
        f = b["filename"][0]
        npz = np.load(tmp_path / "IntRes" / "direct_depthmaps" / "colmap" / "s0" / f"{f}_out.npz")
        dg = read_array(stereo / "depth_maps" / f"{f}.jpg.geometric.bin")
        assert dg.shape == (48, 64) and np.array_equal(dg, npz["depthmap"])
        assert np.array_equal(npz["probability"], np.ones_like(dg))
        ng = read_array(stereo / "normal_maps" / f"{f}.jpg.geometric.bin")
        assert ng.shape == (48, 64, 3) and np.array_equal(ng[dg == 0], np.zeros(((dg == 0).sum(), 3), np.float32))
        dp = read_array(stereo / "depth_maps" / f"{f}.jpg.photometric.bin")
        np_ = read_array(stereo / "normal_maps" / f"{f}.jpg.photometric.bin")
        assert (dp > 0).all() and np.allclose(np.linalg.norm(np_, axis=-1), 1.0, atol=1e-4)
        assert (dg > 0).mean() > 0.3
    # the stored photometric maps are what ops.patch_match computes for the view
    b = batches[1]
    g = [ops.grey_image(im.cuda()) for im in b["imgs"][0]]
    cams = ops.geo_filter_cams(b["K"][0], b["R"][0], b["t"][0]).cuda()
    st = ops.patch_match(g[0], g[1:], cams, float(b["depth_min"][0][0]), float(b["depth_max"][0][0]), num_iterations=3, view=1)
    assert np.array_equal(st[..., 0].cpu().numpy(), read_array(stereo / "depth_maps" / f"{b['filename'][0]}.jpg.photometric.bin"))
    before = sorted(p.stat().st_mtime_ns for p in stereo.rglob("*.bin"))
    assert depthmap_colmap(batches, args) is None                   # returns early: the dense folder exists
    assert sorted(p.stat().st_mtime_ns for p in stereo.rglob("*.bin")) == before


def test_limits(env):
    L, ops, synthetic = env
    sc, greys, cams = _scene(synthetic, ops, 3, 16, 24)
    g = [torch.from_numpy(x).cuda() for x in greys]
    cams = cams.cuda()
    st = ops.patch_match_init(16, 24, cams, 2.0, 8.0)
    run = lambda **kw: ops.patch_match(kw.pop("ref", g[0]), kw.pop("srcs", g[1:]), kw.pop("cams", cams), kw.pop("dmin", 2.0),
                                       kw.pop("dmax", 8.0), num_iterations=1, **kw)
    for kw in [dict(srcs=[]), dict(srcs=[g[1]] * 32, cams=cams[[0] + [1] * 32].contiguous()), dict(dmin=0.0), dict(dmin=-1.0),
               dict(dmin=8.0), dict(dmin=9.0), dict(radius=0), dict(radius=9), dict(step=0), dict(radius=2, step=3), dict(top_k=0),
               dict(top_k=3), dict(cams=cams[:2].contiguous())]:
        with pytest.raises(ValueError):
            run(**kw)
    with pytest.raises(ValueError):
        ops.patch_match_half_step(st, g[0], g[1:], cams, 2.0, 8.0, colour=2, iteration=0, delta=0.1, theta=0.1)
    with pytest.raises(ValueError):
        ops.patch_match_filter(st, g[0], g[1:], cams, None)
    with pytest.raises(ValueError):
        ops.patch_match_cost(st[:8].contiguous(), g[0], g[1:], cams)
    with pytest.raises(RuntimeError):
        run(ref=g[0].cpu())
    with pytest.raises(RuntimeError):
        ops.patch_match_cost(st.cpu(), g[0], g[1:], cams)
    # the C entry points check the same limits themselves
    sptr = (__import__("ctypes").c_void_p * 2)(*[x.data_ptr() for x in g[1:]])
    hw = (__import__("ctypes").c_int * 4)(16, 24, 16, 24)
    lib = L.lib()
    args = lambda S, r, s, k: (st.data_ptr(), g[0].data_ptr(), 16, 24, sptr, hw, S, cams.data_ptr(), None, r, s, k,
                               torch.empty(2, 16, 24, device="cuda").data_ptr(), None, None, ops._stream())
    assert lib.pscv_patch_match_cost(*args(2, 5, 1, 2)) == 0
    for bad in [(0, 5, 1, 1), (32, 5, 1, 1), (2, 0, 1, 1), (2, 9, 1, 1), (2, 5, 6, 1), (2, 5, 1, 3), (2, 5, 1, 0)]:
        assert lib.pscv_patch_match_cost(*args(*bad)) == -1
    assert lib.pscv_patch_match_init(st.data_ptr(), 16, 24, cams.data_ptr(), 3.0, 3.0, 0, 0, ops._stream()) == -1
    torch.cuda.synchronize()
