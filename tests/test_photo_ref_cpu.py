"""The float64 reference of tests/_photo_ref.py and the rigs of tests/_photo_rigs.py, checked WITHOUT a GPU:
  * every rig reaches the regime it is named for and keeps its fragile share under FRAGILE_CAP, from the reference alone;
  * the reference equals oracle/photometric.py and oracle/vismvsnet.py evaluated in float64 (inputs cast; the oracle's fp32 window is
    cast inside this file), i.e. ATen's float64 grid_sample and autograd, on every rig -- non-finite depth included;
  * it equals the reference project's own outputs (tests/golden/photo_*.npz, homography_tiny.npz) at their fp32 tolerance;
  * the ``ops`` wrappers refuse CPU tensors before anything else (their other refusals need a device: tests/test_gpu_photo_ref.py)."""
import os

import numpy as np
import pytest
import torch

import _photo_ref as R
import _photo_rigs as G
from oracle import photometric as P
from oracle import vismvsnet as OV

GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(autouse=True)
def _window64(monkeypatch):
    """The oracle builds its window in fp32; evaluated in float64 it keeps those fp32 VALUES."""
    w32 = P._window
    monkeypatch.setattr(P, "_window", lambda *a, **k: w32(*a, **k).double())


def close(a, b, rtol=1e-9, atol=1e-12, what=""):
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert torch.equal(torch.isnan(a), torch.isnan(b)), f"{what}: NaN positions differ"
    fin = ~torch.isnan(a)
    err = (a[fin] - b[fin]).abs()
    bad = err > atol + rtol * b[fin].abs()
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements differ, worst {float(err.max()):.3e}"


# ---- rigs ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(G.PHOTO_RIGS))
def test_photo_rig_reaches_its_regime_under_the_fragile_cap(name):
    rig = G.photo_rig(name)                                   # asserts the regime
    shares = G.fragile_shares(rig)
    print(f"[rig] {name}: fragile share fwd {shares['fwd']:.4f} mask {shares['mask']:.4f} bwd {shares['bwd']:.4f}")
    assert max(shares.values()) <= R.FRAGILE_CAP, shares


def test_a_rig_that_misses_its_regime_fails():
    rig = G.free((16, 24), 2, 3, 1)
    for check in (G.check_clamp, G.check_part_behind, G.check_z_clamp, G.check_border):
        with pytest.raises(AssertionError):
            check(rig)


def test_fragile_sees_each_decision():
    """Maps built to sit ON the decisions: texel centres (ix = x), |g| = 1 at the outermost pixels, q_z = 0 in column 4."""
    h, w = 5, 8
    eye = torch.eye(4).view(1, 4, 4)
    depth = torch.ones(1, h, w)
    on_texels = torch.tensor([[(w - 1) / w, 0.0, 0.5 * (w - 1) / w, 0.0], [0.0, 0.75, 0.3, 0.0], [0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 1.0]])
    f = R.fragile(depth, eye, on_texels.view(1, 1, 4, 4))
    assert bool(f["bwd"].all()) and not bool(f["fwd"].any())
    f = R.fragile(depth, eye, eye.view(1, 1, 4, 4))                               # f = (x, y): g = -1 at 0, +1 at size - 1
    edge = torch.zeros(h, w, dtype=torch.bool)
    edge[0], edge[-1], edge[:, 0], edge[:, -1] = True, True, True, True
    assert torch.equal(f["mask"][0, 0], edge)
    cut = eye.clone().view(1, 1, 4, 4)
    cut[0, 0, 2, 0] = -0.25
    f = R.fragile(depth, eye, cut)
    assert bool(f["fwd"][0, 0, :, 4].all()) and int(f["fwd"].sum()) == h


def test_non_finite_image_rig_has_no_sample_near_an_integer_position():
    rig = G.non_finite_image()
    assert G.fragile_shares(rig)["bwd"] == 0.0


@pytest.mark.parametrize("case", G.HOMOG_CASES, ids=lambda c: f"{c[0]}-pp{c[1]}-c{c[2]}")
def test_homography_rig_reaches_its_regime(case):
    G.homog(*case)                                            # check_homog inside
    for exact in (True, False):
        G.collision(exact)


# ---- photo warp against the oracle / ATen in float64 ----------------------------------------------------------------------------------
def _aten(rig, with_grad=True):
    """oracle/photometric.py in float64 on a rig: flows, z, mask, warped, warped_depth, and d sum(grad warped) / d depth."""
    B, S, C, h, w = rig["src"].shape
    inv_ref, proj = rig["inv_ref"].double(), rig["proj"].double()
    pm = torch.cat((torch.linalg.inv(inv_ref).unsqueeze(1), proj), dim=1)
    depth = rig["depth"].double().clone().requires_grad_(with_grad)
    flows, z = P.get_flow_from_depthmap(depth, pm, (h, w), 0)
    mask = ((flows < 1).all(dim=-1) & (flows > -1).all(dim=-1)).double()
    gs = lambda x, s: torch.nn.functional.grid_sample(x, flows[:, s], mode="bilinear", padding_mode="zeros", align_corners=False)
    warped = torch.stack([gs(rig["src"][:, s].double(), s) for s in range(S)], dim=1)
    wd = torch.stack([gs(rig["src_depth"][:, s:s + 1].double(), s)[:, 0] for s in range(S)], dim=1)
    grad = None
    if with_grad:
        (warped * rig["grad"].double()).sum().backward()
        grad = depth.grad
    return flows.detach(), z.detach(), mask, warped.detach(), wd.detach(), grad


@pytest.mark.parametrize("name", sorted(G.PHOTO_RIGS))
def test_photo_reference_is_aten_in_float64(name):
    rig = G.photo_rig(name)
    flows, z, mask, warped, wd, grad = _aten(rig)
    r = R.photo_warp(rig["src"], rig["depth"], rig["inv_ref"], rig["proj"], rig["src_depth"])
    # inverse(inverse(inv_ref)) and 1e-6 against its fp32 value: 1e-7 relative in the z-clamp band, 1e-12 elsewhere
    rt = 2e-7 if name == "z_clamp" else 1e-9
    close(r["z"], z, rtol=rt, atol=1e-18, what="z")
    close(r["flows"], flows, rtol=rt, atol=1e-7 if name == "z_clamp" else 1e-9, what="flows")
    assert torch.equal(r["mask"], mask)
    close(r["warped"], warped, rtol=rt, atol=1e-6 if name == "z_clamp" else 1e-9, what="warped")
    close(r["warped_depth"], wd, rtol=rt, atol=1e-6 if name == "z_clamp" else 1e-9, what="warped_depth")
    b = R.warp_bwd(rig["src"], rig["depth"], rig["inv_ref"], rig["proj"], rig["grad"])
    close(b["grad"], grad, rtol=1e-6 if name == "z_clamp" else 1e-8, atol=1e-8 * float(grad.abs().max()), what="grad_depth")
    assert bool((b["U"] >= 0).all()) and bool(torch.isfinite(b["U"]).all()) and bool((b["coarse"] >= b["grad"].abs()).all())
    assert bool(torch.isfinite(r["Uwarped"]).all()) and bool((r["Uwarped"] >= r["warped"].abs() * 0.999).all())


def test_non_finite_depth_behaves_like_aten():
    """The decision of the NaN case: torch.clamp propagates NaN, grid_sample returns NaN at a NaN coordinate and its backward a NaN
    depth gradient; the mask is 0 there.  -inf depth at a pixel whose point then lies behind goes to -10 like any z <= 0."""
    rig = G.non_finite_depth()
    flows, z, mask, warped, wd, grad = _aten(rig)
    r = R.photo_warp(rig["src"], rig["depth"], rig["inv_ref"], rig["proj"], rig["src_depth"])
    b = R.warp_bwd(rig["src"], rig["depth"], rig["inv_ref"], rig["proj"], rig["grad"])
    bad = ~torch.isfinite(rig["depth"])
    assert int(bad.sum()) == 7
    nanpix = torch.isnan(r["flows"]).any(-1)
    assert int(nanpix.sum()) >= 4 and bool((r["mask"][nanpix] == 0).all())
    assert bool(torch.isnan(r["warped"].permute(0, 1, 3, 4, 2)[nanpix]).all()) and bool(torch.isnan(r["warped_depth"][nanpix]).all())
    assert not bool(torch.isnan(r["warped"].permute(0, 1, 3, 4, 2)[~nanpix]).any())
    close(r["z"], z, what="z")
    close(r["flows"], flows, atol=1e-9, what="flows")
    assert torch.equal(r["mask"], mask)
    close(r["warped"], warped, atol=1e-9, what="warped")
    close(r["warped_depth"], wd, atol=1e-9, what="warped_depth")
    close(b["grad"], grad, rtol=1e-8, atol=1e-9, what="grad_depth")
    assert bool(torch.isnan(b["grad"][nanpix.any(1)]).all()) and int(torch.isnan(b["grad"]).sum()) == int(nanpix.any(1).sum())


def test_non_finite_image_behaves_like_aten():
    rig = G.non_finite_image()
    flows, z, mask, warped, wd, grad = _aten(rig)
    r = R.photo_warp(rig["src"], rig["depth"], rig["inv_ref"], rig["proj"], rig["src_depth"])
    for got, want in ((r["warped"], warped), (r["warped_depth"], wd)):
        assert torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(torch.isinf(got), torch.isinf(want))
        assert int(torch.isnan(got).sum()) >= 2 and int(torch.isinf(got).sum()) >= 2
    b = R.warp_bwd(rig["src"], rig["depth"], rig["inv_ref"], rig["proj"], rig["grad"])
    assert torch.equal(torch.isfinite(b["grad"]), torch.isfinite(grad)) and int((~torch.isfinite(grad)).sum()) >= 4


# ---- SSIM -----------------------------------------------------------------------------------------------------------------------------
def test_window_is_the_kernels():
    g = R.window()
    assert g.dtype == torch.float64 and torch.equal(g, g.float().double()) and torch.equal(g, g.flip(0))
    assert abs(float(g.sum()) - 1.0) < 3e-7
    o = P._window(channel=1)[0, 0]
    assert float((torch.outer(g, g) - o).abs().max()) < 1e-8           # the oracle's fp32 window: the same up to fp32 rounding


@pytest.mark.parametrize("kind", G.SSIM_KINDS)
def test_ssim_reference_is_the_oracle_in_float64(kind):
    cases = G.ssim_cases(kind)
    if kind == "random":
        cases = cases[::5]
    for h, w, n1, rep, C in cases:
        a, b, go = G.ssim_inputs(kind, h, w, n1, rep, C)
        bb = b.double().clone().requires_grad_(True)
        want = P.ssim_loss(a.double().repeat_interleave(rep, dim=0), bb)
        want.backward(go.double())
        r = R.ssim(a, b, rep)
        # the two windows differ by fp32 roundings (2e-8 per weight): a few 1e-7 U at most
        tol = 64 * R.EPS * r["U"]
        nan = torch.isnan(r["out"])
        assert torch.equal(nan, torch.isnan(want)), (kind, h, w)
        assert bool(((r["out"] - want.detach()).abs()[~nan] <= tol[~nan]).all()), (kind, h, w, float((r["out"] - want.detach()).abs()[~nan].max()))
        gb = R.ssim_bwd(a, b, go, rep)
        gnan = torch.isnan(gb["grad"])
        assert torch.equal(gnan, torch.isnan(bb.grad)), (kind, h, w)
        assert bool(((gb["grad"] - bb.grad).abs()[~gnan] <= 64 * R.EPS * gb["U"][~gnan]).all()), (kind, h, w)
        if kind == "zeros":
            assert float(r["out"].abs().max()) == 0.0 and bool(torch.isfinite(gb["grad"]).all())
        if kind == "equal":
            assert float(r["out"].abs().max()) < 1e-12
        if kind == "nan":                                     # the 11 x 11 neighbourhood of the NaN pixel and nothing else
            want_nan = torch.zeros_like(nan)
            y, x = h // 2, w // 2
            want_nan[-1, C - 1, max(0, y - 5):y + 6, max(0, x - 5):x + 6] = True
            assert torch.equal(nan, want_nan)


def test_ssim_backward_is_autograd_of_the_reference_forward():
    """The analytic (dS/dmu2, dS/dE22, dS/dE12) against autograd through the reference's OWN forward (same window: 1e-10)."""
    for h, w, n1, rep, C in ((9, 33, 2, 3, 3), (3, 5, 1, 1, 1), (17, 31, 3, 1, 4)):
        a, b, go = G.ssim_inputs("random", h, w, n1, rep, C, seed=3)
        bb = b.double().requires_grad_(True)
        R.ssim(a, bb, rep)["out"].backward(go.double())
        close(R.ssim_bwd(a, b, go, rep)["grad"], bb.grad, rtol=1e-9, atol=1e-12, what="ssim_bwd")


# ---- goldens --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["photo_tiny", "photo_behind"])
def test_reference_composition_matches_the_reference_projects_golden(tag):
    from wild_deep_mvs_amd import synthetic
    g = np.load(os.path.join(GOLD, f"{tag}.npz"))
    B, V, H, W, seed, behind, masked, i_ref = [int(v) for v in g["meta"]]
    sc = synthetic.make_photo_case(B, V, H, W, seed=seed, behind_view=behind)
    proj = torch.from_numpy(g["proj"]).double()
    comp = R.photometricloss(sc["imgs"], sc["depths"][0], torch.linalg.inv(proj[:, 0]), proj[:, 1:])
    # no sample is anywhere near q_z = 0 (100 margins away at least): tests/test_gpu_photo.py relies on it with the device's inverse
    fl = R.flows(sc["depths"][0], torch.linalg.inv(proj[:, 0]), proj[:, 1:])
    assert float((fl["z"].abs() / (R.POS_RATIO * R.EPS * fl["Uz"])).min()) > 100.0
    moved = float((comp["mask"].numpy() != g["mask"]).mean())
    err = np.abs(comp["ssim"].numpy() - g["ssim"])
    rel = np.abs(comp["grad_depth"].numpy() - g["grad_depth"]).sum() / np.abs(g["grad_depth"]).sum()
    print(f"[pin] {tag}: ssim max abs {err.max():.2e}, mask flips {moved:.2e}, loss {float(comp['loss']):.7f} vs {float(g['loss']):.7f}, grad rel-L1 {rel:.2e}")
    assert moved <= 1e-3 and err.max() <= 1e-4 and abs(float(comp["loss"]) - float(g["loss"])) <= 1e-5 and rel <= 1e-4


def test_homography_reference_matches_the_golden():
    g = np.load(os.path.join(GOLD, "homography_tiny.npz"))
    t = lambda k: torch.from_numpy(g[k])
    src, Hp, wgt = t("src"), t("H_pixel"), t("weight")
    h, w = g["warped"].shape[2:]
    r = R.homography(src.permute(0, 2, 3, 1), Hp, (h, w))
    gb = R.homography_bwd(wgt.permute(0, 2, 3, 1), Hp, src.shape[2:])
    assert float((r["out"].permute(0, 3, 1, 2) - t("warped").double()).abs().max()) <= 3e-4
    assert float((gb["grad"].permute(0, 3, 1, 2) - t("grad_src").double()).abs().max()) <= 3e-4


# ---- homography against the oracle in float64 -------------------------------------------------------------------------------------------
def _oracle_homography(rig):
    img = rig["img"].double().permute(0, 3, 1, 2).clone().requires_grad_(True)
    H = rig["H"].double()
    if H.dim() == 3:
        H = H.view(-1, 1, 1, 3, 3)
    # the oracle's pixel grid is an explicit fp32 arange (exact values): inside ITS module only, `torch.arange(dtype=float32)` is float64
    class _Torch64:
        def __getattr__(self, name):
            return getattr(torch, name)

        @staticmethod
        def arange(*a, **k):
            return torch.arange(*a, **{**k, "dtype": torch.float64} if k.get("dtype") == torch.float32 else k)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(OV, "torch", _Torch64())
        out = OV.homography_warping(img, H, rig["ref_hw"])
    (out * rig["grad"].double().permute(0, 3, 1, 2)).sum().backward()
    return out.detach().permute(0, 2, 3, 1), img.grad.permute(0, 2, 3, 1)


def _pin_homography(rig, rtol=1e-9):
    want, wgrad = _oracle_homography(rig)
    r = R.homography(rig["img"], rig["H"], rig["ref_hw"])
    gb = R.homography_bwd(rig["grad"], rig["H"], rig["src_hw"])
    close(r["out"], want, rtol=rtol, atol=1e-7 if rtol > 1e-9 else 1e-10, what=rig["name"])
    close(gb["grad"], wgrad, rtol=rtol, atol=1e-6 if rtol > 1e-9 else 1e-9, what=rig["name"] + " adjoint")
    assert bool((gb["U"] >= gb["grad"].abs() * 0.999).all())


@pytest.mark.parametrize("case", G.HOMOG_CASES, ids=lambda c: f"{c[0]}-pp{c[1]}-c{c[2]}")
def test_homography_reference_is_the_oracle_in_float64(case):
    _pin_homography(G.homog(*case), rtol=2e-7 if case[0] == "tiny_z" else 1e-9)      # 1e-9 against its fp32 value in the band


@pytest.mark.parametrize("sizes", G.HOMOG_SMALL, ids=str)
def test_homography_oracle_is_defined_at_one_texel_wide_sources(sizes):
    """hs or ws = 1: align_corners=True maps every normalised coordinate to texel 0 ((g + 1) / 2 (1 - 1) = 0), in the oracle as in
    the kernel's (ws - 1) / ws scale: the sizes stay in the GPU test."""
    ref_hw, src_hw = sizes
    for pp in (0, 1):
        rig = G.homog("free", pp, 3, ref_hw=ref_hw, src_hw=src_hw)
        want, _ = _oracle_homography(rig)
        assert bool(torch.isfinite(want).all())
        _pin_homography(rig)


def test_collision_rigs_against_the_oracle():
    for exact in (True, False):
        _pin_homography(G.collision(exact))
    rig = G.collision(True)
    gb = R.homography_bwd(rig["grad"], rig["H"], rig["src_hw"])["grad"]
    assert torch.equal(gb, gb.float().double()) and torch.equal(gb * 4, torch.round(gb * 4)) and float(gb.abs().max()) < 2 ** 22


# ---- wrappers ---------------------------------------------------------------------------------------------------------------------------
def test_ops_wrappers_refuse_cpu_tensors():
    """There is no CPU fall-back: the device check comes first in every wrapper."""
    from wild_deep_mvs_amd import ops
    rig = G.free((5, 7), 1, 1, 1)
    a = torch.rand(1, 1, 5, 7)
    for call in (lambda: ops.photo_warp(rig["src"], rig["depth"], rig["inv_ref"], rig["proj"]),
                 lambda: ops.photo_warp_bwd(rig["src"], rig["depth"], rig["inv_ref"], rig["proj"], rig["grad"]),
                 lambda: ops.ssim(a, a), lambda: ops.ssim_bwd(a, a, a),
                 lambda: ops.homography_warp(torch.rand(1, 4, 4, 2), torch.eye(3).view(1, 3, 3), (4, 4)),
                 lambda: ops.homography_warp_bwd(torch.rand(1, 4, 4, 2), torch.eye(3).view(1, 3, 3), (4, 4))):
        with pytest.raises(RuntimeError, match="MI355X only"):
            call()
