"""The kernels of the unsupervised training path -- photo_warp_kernel, photo_warp_bwd_kernel, ssim_kernel<0|1>, ssim_bwd_finish_kernel
(csrc/photo_loss.hip) and homography_warp_kernel, homography_warp_bwd_kernel (csrc/homog_warp.hip) -- called through their ``ops``
wrappers and held, element by element, to the float64 reference of tests/_photo_ref.py on the hand-written rigs of
tests/_photo_rigs.py (tests/test_photo_ref_cpu.py checks both without a GPU).

What is asserted, per element:  |got - ref| <= BOUND 2^-24 U  with the unit U of _photo_ref.py (absolute values, first order).
BOUND is 4 x the worst ratio measured on an MI355X (DESIGN.md holds the table), never above the count of roundings in the kernel's
chain (``CAP``):
  z, flows, warped, warped_depth   9    x d (1) + two 4-term dot products (4 + 4); every later operation rounds once and stands in U once
  photo_warp_bwd                   9 + C + S + 6   the position chain, the channel and view sums, slope (3) and scale (3) arithmetic
  ssim                             23   a square (1) + 11 + 11 fused multiply-adds of the separable blur; the scalar chain stands in U
  ssim_bwd                         45   the same, and the second blur's 22
  homography_warp                  7    weights (3) + product (1) + sum of four (3); the position's 3 roundings are fewer
  homography_warp_bwd              N + 4   N = the largest number of contributions to one texel (an fp32 sum of N terms in any order)
The mask is exact outside ``fragile``; fragile elements (at most FRAGILE_CAP of a rig, asserted on the CPU) keep their class and a
coarse bound.  NaN and inf stand exactly where the reference has them."""
import itertools

import pytest
import torch

import _photo_cmp as PC
import _photo_ref as R
import _photo_rigs as G
from _photo_cmp import BOUND, EPS

pytestmark = pytest.mark.gpu


WORST = {}


def compare(*a, **k):
    return PC.compare(*a, table=WORST, **k)


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from wild_deep_mvs_amd import _lib as L, ops
    L.lib()
    yield L, ops
    print("\n[parity] photo ref: worst |got - ref| / (2^-24 U) per kernel and output", flush=True)
    for (kern, out), v in sorted(WORST.items()):
        print(f"[parity] photo ref worst {kern:20s} {out:13s} {v:.3f} (bound {BOUND[(kern, out)]})", flush=True)


def _dev(rig, *keys):
    return [rig[k].cuda().contiguous() for k in keys]


def check_photo_rig(ops, rig, tag=None):
    """Every output of one pscv_photo_warp launch and pscv_photo_warp_bwd on a rig."""
    tag = tag or rig["name"]
    src, depth, inv_ref, proj, sd, gw = _dev(rig, "src", "depth", "inv_ref", "proj", "src_depth", "grad")
    o = ops.photo_warp(src, depth, inv_ref, proj, src_depth=sd, want_mask=True, want_z=True, want_flows=True)
    gd = ops.photo_warp_bwd(src, depth, inv_ref, proj, gw)
    torch.cuda.synchronize()
    r = R.photo_warp(rig["src"], rig["depth"], rig["inv_ref"], rig["proj"], rig["src_depth"])
    f = R.fragile(rig["depth"], rig["inv_ref"], rig["proj"])
    B, S, C, h, w = rig["src"].shape
    compare(("photo_warp", "z"), f"{tag} z", o["z"], r["z"], r["Uz"])
    fl = r["flows"]
    compare(("photo_warp", "flows"), f"{tag} flows", o["flows"], fl, r["Uflows"], exempt=f["fwd"].unsqueeze(-1).expand_as(fl),
            coarse=(fl + 10.0).abs() + 1e-3)                                  # q_z ~ 0: the reference's value or -10
    top = float(rig["src"][torch.isfinite(rig["src"])].abs().max())
    ex = f["fwd"].unsqueeze(2).expand(B, S, C, h, w)
    compare(("photo_warp", "warped"), f"{tag} warped", o["warped"], r["warped"], r["Uwarped"], exempt=ex,
            coarse=torch.full_like(r["warped"], 2.0 * top))
    compare(("photo_warp", "warped_depth"), f"{tag} warped_depth", o["warped_depth"], r["warped_depth"], r["Uwarped_depth"],
            exempt=f["fwd"], coarse=torch.full_like(r["warped_depth"], 2.0 * float(rig["src_depth"][torch.isfinite(rig["src_depth"])].abs().max())))
    got_mask = o["mask"].double().cpu()
    assert bool(((got_mask == 0) | (got_mask == 1)).all())
    assert torch.equal(got_mask[~f["mask"]], r["mask"][~f["mask"]]), f"{tag}: mask differs outside the fragile set"
    b = R.warp_bwd(rig["src"], rig["depth"], rig["inv_ref"], rig["proj"], rig["grad"])
    compare(("photo_warp_bwd", "grad_depth"), f"{tag} grad_depth", gd, b["grad"], b["U"], cap=9 + C + S + 6, exempt=f["bwd"].any(dim=1),
            coarse=b["coarse"] + BOUND[("photo_warp_bwd", "grad_depth")] * EPS * b["U"])
    return o, gd


@pytest.mark.parametrize("name", sorted(G.PHOTO_RIGS))
def test_photo_warp_and_backward_on_rig(env, name):
    L, ops = env
    check_photo_rig(ops, G.photo_rig(name))


def test_photo_warp_every_output_combination(env):
    """Every set of outputs ops.photo_warp can be asked for -- the calls without images (C = 0) of Trainer.get_flow_from_depthmap and
    of the masked loss among them -- writes exactly the requested maps, bit for bit those of the all-outputs launch that
    test_photo_warp_and_backward_on_rig holds to the reference."""
    L, ops = env
    rig = G.photo_rig("free_5x7_S4_C3_B3")
    src, depth, inv_ref, proj, sd = _dev(rig, "src", "depth", "inv_ref", "proj", "src_depth")
    full, _ = check_photo_rig(ops, rig)
    empty = src[:, :, :0].contiguous()
    for imgs, with_sd, m, z, fl in itertools.product((src, None, empty), (True, False), (True, False), (True, False), (True, False)):
        o = ops.photo_warp(imgs, depth, inv_ref, proj, src_depth=sd if with_sd else None, want_mask=m, want_z=z, want_flows=fl)
        want = {"warped": imgs is not None, "mask": m, "z": z, "flows": fl, "warped_depth": with_sd}
        for k, asked in want.items():
            assert (o[k] is not None) == asked, (k, want)
            if asked and not (k == "warped" and imgs is empty):
                assert torch.equal(o[k].view(torch.int32), full[k].view(torch.int32)), (k, want)
        if imgs is empty:
            assert tuple(o["warped"].shape) == (3, 4, 0, 5, 7)


def test_non_finite_depth_propagates_like_aten(env):
    """NaN, +inf and -inf depth pixels (column 0 included, where x inf = NaN): flows, warped, warped_depth and grad_depth are NaN
    exactly where the float64 reference (= ATen, test_photo_ref_cpu.py) has NaN, the mask is 0 there, every other pixel is untouched."""
    L, ops = env
    rig = G.non_finite_depth()
    o, gd = check_photo_rig(ops, rig)
    r = R.photo_warp(rig["src"], rig["depth"], rig["inv_ref"], rig["proj"])
    nanpix = torch.isnan(r["flows"]).any(-1)
    assert int(nanpix.sum()) >= 4
    assert bool((o["mask"].cpu()[nanpix] == 0).all()) and bool(torch.isnan(gd.cpu()[nanpix.any(1)]).all())


def test_non_finite_texels_reach_exactly_the_samples_that_touch_them(env):
    L, ops = env
    rig = G.non_finite_image()
    o, gd = check_photo_rig(ops, rig)
    assert int(torch.isnan(o["warped"]).sum()) >= 2 and int(torch.isinf(o["warped"]).sum()) >= 2
    assert int((~torch.isfinite(gd)).sum()) >= 4


def test_photo_warp_refusals(env):
    L, ops = env
    rig = G.free((5, 7), 2, 3, 1)
    src, depth, inv_ref, proj, sd, gw = _dev(rig, "src", "depth", "inv_ref", "proj", "src_depth", "grad")
    for hh, ww in ((1, 7), (5, 1)):                                   # (size - 1) normalisation: h = 1 or w = 1 has no flow
        with pytest.raises(L.PscvError, match="bad sizes"):
            ops.photo_warp(src[..., :hh, :ww].contiguous(), depth[:, :hh, :ww].contiguous(), inv_ref, proj)
        with pytest.raises(L.PscvError, match="bad sizes"):
            ops.photo_warp_bwd(src[..., :hh, :ww].contiguous(), depth[:, :hh, :ww].contiguous(), inv_ref, proj, gw[..., :hh, :ww].contiguous())
    with pytest.raises(L.PscvError, match="null pointer|bad sizes"):  # a backward without channels
        ops.photo_warp_bwd(src[:, :, :0].contiguous(), depth, inv_ref, proj, gw[:, :, :0].contiguous())
    for bad in (lambda: ops.photo_warp(src.double(), depth, inv_ref, proj), lambda: ops.photo_warp(src, depth.half(), inv_ref, proj),
                lambda: ops.photo_warp(src[:, :1].contiguous(), depth, inv_ref, proj),
                lambda: ops.photo_warp(src[..., :4, :].contiguous(), depth, inv_ref, proj),
                lambda: ops.photo_warp(src, depth, inv_ref[:, :3].contiguous(), proj), lambda: ops.photo_warp(src, depth, inv_ref, proj[:, 0].contiguous()),
                lambda: ops.photo_warp(src, depth, inv_ref, proj, src_depth=sd[:, :1].contiguous()),
                lambda: ops.photo_warp(src, depth, inv_ref, proj, src_depth=sd.double()),
                lambda: ops.photo_warp_bwd(src, depth, inv_ref, proj, gw[:, :, :2].contiguous()),
                lambda: ops.photo_warp_bwd(src, depth, inv_ref, proj, gw.double())):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(ValueError, match="contiguous"):
        ops.photo_warp(src, depth.transpose(1, 2), inv_ref, proj)


# ---- SSIM -----------------------------------------------------------------------------------------------------------------------------
def check_ssim(ops, tag, a, b, go, rep):
    out = ops.ssim(a.cuda(), b.cuda())
    g2 = ops.ssim_bwd(a.cuda(), b.cuda(), go.cuda())
    torch.cuda.synchronize()
    r, gb = R.ssim(a, b, rep), R.ssim_bwd(a, b, go, rep)
    compare(("ssim", "out"), f"ssim {tag}", out, r["out"], r["U"])
    compare(("ssim_bwd", "grad"), f"ssim_bwd {tag}", g2, gb["grad"], gb["U"])
    return out, g2, r, gb


@pytest.mark.parametrize("kind", G.SSIM_KINDS)
def test_ssim_and_backward(env, kind):
    """h in {1,3,7,8,9,17} x w in {1,5,31,32,33,65} (images smaller than the 11-tap window, both edges of the 32 x 8 tile), C in
    {1,3,4}, (n1, rep) in {(1,1),(2,3),(3,1)} on random images; equal, constant, all-zero, 0..255-scale and one-NaN-pixel images at
    three sizes."""
    L, ops = env
    for h, w, n1, rep, C in G.ssim_cases(kind):
        a, b, go = G.ssim_inputs(kind, h, w, n1, rep, C)
        out, g2, r, gb = check_ssim(ops, f"{kind} {h}x{w} n1={n1} rep={rep} C={C}", a, b, go, rep)
        if kind == "zeros":                                   # S = 1 exactly: (C1 C2) / (C1 C2), the same fp32 number twice
            assert float(out.abs().max()) == 0.0 and bool(torch.isfinite(g2).all())
        if kind == "nan":
            want = torch.zeros(n1 * rep, C, h, w, dtype=torch.bool)
            y, x = h // 2, w // 2
            want[-1, C - 1, max(0, y - 5):y + 6, max(0, x - 5):x + 6] = True
            assert torch.equal(torch.isnan(out).cpu(), want)


def test_ssim_plane_limit(env):
    """The grid's z extent: n1 rep C = 65535 planes of 1 x 1 run (and are right); 65536 are refused."""
    L, ops = env
    g = torch.Generator().manual_seed(12)
    a, b, go = torch.rand(4369, 3, 1, 1, generator=g), torch.rand(4369 * 5, 3, 1, 1, generator=g), torch.randn(4369 * 5, 3, 1, 1, generator=g)
    assert b.shape[0] * b.shape[1] == 65535
    check_ssim(ops, "65535 planes of 1x1", a, b, go, 5)
    a, b = torch.rand(4096, 4, 1, 1, generator=g).cuda(), torch.rand(4096 * 4, 4, 1, 1, generator=g).cuda()
    with pytest.raises(L.PscvError, match="bad sizes"):
        ops.ssim(a, b)
    with pytest.raises(L.PscvError, match="bad sizes"):
        ops.ssim_bwd(a, b, torch.ones_like(b))


def test_ssim_refusals(env):
    L, ops = env
    a, b = torch.rand(2, 3, 5, 7).cuda(), torch.rand(4, 3, 5, 7).cuda()
    for bad in (lambda: ops.ssim(a, b[:3].contiguous()),              # img2.shape[0] % n1
                lambda: ops.ssim(a, b[:, :2].contiguous()), lambda: ops.ssim(a, b[..., :6].contiguous()), lambda: ops.ssim(a.double(), b),
                lambda: ops.ssim(a, b.half()), lambda: ops.ssim(a[0], b), lambda: ops.ssim_bwd(a, b, b[:2].contiguous()),
                lambda: ops.ssim_bwd(a, b, b.double()), lambda: ops.ssim_bwd(a, b[:3].contiguous(), b[:3].contiguous())):
        with pytest.raises(ValueError):
            bad()


# ---- homography -----------------------------------------------------------------------------------------------------------------------
def check_homography(ops, rig):
    img, H, go = _dev(rig, "img", "H", "grad")
    out = ops.homography_warp(img, H, rig["ref_hw"])
    gi = ops.homography_warp_bwd(go, H, rig["src_hw"])
    torch.cuda.synchronize()
    r, gb = R.homography(rig["img"], rig["H"], rig["ref_hw"]), R.homography_bwd(rig["grad"], rig["H"], rig["src_hw"])
    compare(("homography_warp", "out"), rig["name"], out, r["out"], r["U"])
    compare(("homography_warp_bwd", "grad"), rig["name"] + " adjoint", gi, gb["grad"], gb["U"], cap=PC.contributions(rig["H"], rig["ref_hw"], rig["src_hw"]) + 4)
    return gi, gb


@pytest.mark.parametrize("case", G.HOMOG_CASES, ids=lambda c: f"{c[0]}-pp{c[1]}-c{c[2]}")
def test_homography_warp_and_adjoint(env, case):
    L, ops = env
    check_homography(ops, G.homog(*case))


@pytest.mark.parametrize("sizes", G.HOMOG_SMALL, ids=str)
def test_homography_warp_small_sources(env, sizes):
    L, ops = env
    for pp in (0, 1):
        check_homography(ops, G.homog("free", pp, 3, ref_hw=sizes[0], src_hw=sizes[1]))


def test_homography_adjoint_under_collisions(env):
    """960 reference pixels scatter into the same four texels.  Exact variant: weights in {0, 0.25, 0.5, 1} and integer gradients,
    every partial sum exact in fp32 -- the result is bit for bit the reference's under ANY order of the atomic adds.  Real variant:
    held to the unit sum |g w| like every other case."""
    L, ops = env
    rig = G.collision(True)
    gi, gb = check_homography(ops, rig)
    assert torch.equal(gi.double().cpu(), gb["grad"]), "the exact collision case must not depend on the order of the atomic adds"
    assert int((gb["grad"] != 0).sum()) >= 8
    check_homography(ops, G.collision(False))


def test_homography_refusals(env):
    L, ops = env
    img, H = torch.rand(2, 4, 5, 3).cuda(), torch.eye(3).repeat(2, 1, 1).cuda()
    with pytest.raises(TypeError):
        ops.homography_warp(img.double(), H, (4, 5))
    with pytest.raises(TypeError):
        ops.homography_warp(img, H.double(), (4, 5))
    with pytest.raises(ValueError):
        ops.homography_warp(img, H[:1].contiguous(), (4, 5))
    with pytest.raises(ValueError):
        ops.homography_warp(img, H.view(2, 1, 1, 3, 3).repeat(1, 4, 5, 1, 1), (4, 6))
    with pytest.raises(L.PscvError):
        ops.homography_warp(img, H, (0, 5))
    with pytest.raises(ValueError):
        ops.homography_warp_bwd(img, H[:1].contiguous(), (4, 5))


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["clamp", "part_behind"])
def test_trainer_photometricloss_against_the_reference_composition(env, name):
    """Trainer.photometricloss (photo_warp -> ssim, autograd: ssim_bwd -> photo_warp_bwd) and the masked mean on a rig, against the
    float64 composition of the same pieces: ssim [B,S,h,w], mask and d loss / d depth per element.  The units carry the upstream
    units along (the warped image's into SSIM, the SSIM gradient's into the warp backward), each scaled by its own kernel's bound."""
    L, ops = env
    from wild_deep_mvs_amd.models.trainer import Trainer
    rig = G.photo_rig(name)
    B, S, C, h, w = rig["src"].shape
    g = torch.Generator().manual_seed(5)
    imgs = torch.cat((torch.rand(B, 1, C, h, w, generator=g), rig["src"]), dim=1)
    pm = torch.cat((torch.linalg.inv(rig["inv_ref"].double()).float().unsqueeze(1), rig["proj"]), dim=1)
    inv_ref = ops.inv_proj4x4(pm[:, 0].cuda().contiguous()).cpu()                 # the values the kernels receive
    depth = rig["depth"].cuda().requires_grad_(True)
    ssim, mask = Trainer().photometricloss(imgs.cuda(), depth, pm.cuda())
    loss = torch.sum(ssim * mask) / torch.sum(mask)
    loss.backward()
    kb = lambda k, o: BOUND[(k, o)]
    comp = R.photometricloss(imgs, rig["depth"], inv_ref, rig["proj"],
                             up=(kb("photo_warp", "warped") / kb("ssim", "out"), kb("ssim_bwd", "grad") / kb("photo_warp_bwd", "grad_depth")))
    f = R.fragile(rig["depth"], inv_ref, rig["proj"])
    G.PHOTO_RIGS[name][1]({**rig, "inv_ref": inv_ref})                            # still the regime it is named for
    assert float(f["mask"].double().mean()) == 0.0                                # no mask decision is in doubt: the mask is exact
    assert torch.equal(mask.double().cpu(), comp["mask"]) and 0 < float(comp["mask"].mean()) < 1
    assert not bool(f["fwd"].any())                                               # nor any q_z = 0 decision: ssim has no exemption
    compare(("photometricloss", "ssim"), f"photometricloss {name} ssim", ssim, comp["ssim"], comp["Ussim"])
    compare(("photometricloss", "grad_depth"), f"photometricloss {name} grad_depth", depth.grad, comp["grad_depth"], comp["Ugrad"],
            cap=9 + C + S + 6, exempt=f["bwd"].any(dim=1), coarse=comp["coarse"] + BOUND[("ssim_bwd", "grad")] * EPS * comp["Ugrad"])
    assert abs(float(loss) - float(comp["loss"])) <= kb("ssim", "out") * EPS * float((comp["Ussim"] * comp["mask"]).sum() / comp["mask"].sum()) + 4 * EPS
