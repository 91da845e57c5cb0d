"""CVP-MVSNet mirror on the HIP engine vs the reference golden (tests/golden/cvp_tiny.npz)."""
import numpy as np
import pytest
import torch

from _util import check_close, load_golden, t
from test_oracle_cvp import cvp_scene

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from wild_deep_mvs_amd import _lib as L, ops, synthetic
    from wild_deep_mvs_amd.models.CVP_MVSNet.frontend import Frontend
    return L, ops, synthetic, Frontend


@pytest.mark.parametrize("fixture", ["cvp_tiny.npz", "cvp_peaked.npz"])
@pytest.mark.parametrize("feature_engine", ["pscv", "torch"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_cvp_forward_parity_with_reference(env, dtype, feature_engine, fixture):
    """Full forward vs the reference golden, with the 2-D pyramid tower on the HIP conv2d kernels (default) and on
    PyTorch-ROCm.  ``cvp_peaked.npz`` (round 6): the same net with its 1-channel head scaled by 4, so that the COARSE level's softmax
    over 96 planes is peaked too (mean max-probability 0.29 against 0.05) and its depth really depends on the cost volume."""
    L, ops, synthetic, Frontend = env
    from test_oracle_cvp import cvp_weights
    g = load_golden(fixture)
    scene, nscale, seed = cvp_scene(g)
    net = Frontend()
    net.load_state_dict(cvp_weights(g, synthetic.template_of(net), seed), strict=True)
    net.storage_dtype = dtype
    net.feature_engine = feature_engine
    net = net.cuda().eval()
    dev = {k: v.cuda() for k, v in scene.items()}
    taps = {}
    out = net(dev["imgs"], dev["K"], dev["R"], dev["t"], dev["depth_min"], dev["depth_max"], nscale=nscale, taps=taps)
    H, W = scene["imgs"].shape[-2:]
    assert tuple(out["depth"].shape) == (1, H, W) and tuple(out["photometric_confidence"].shape) == (1, 1, H, W)
    assert out["depth_pair_list"] == [] and len(out["depth_est_list"]) == nscale
    # intermediate tensors: relative-L2 bars at ~2 x the values measured in round 6 on both fixtures (before: 2e-3 / 6e-3 / 2e-2 in fp16 and
    # 1.5e-2 / 4.5e-2 / 1.5e-1 in bf16) -- fp16 cost 3.2e-4 ... 5.1e-4, coarse logits 7.2e-4 ... 8.4e-4, refinement logits 7.9e-4 ... 9.6e-4;
    # bf16 2.6e-3 ... 4.4e-3, 4.3e-3 ... 4.5e-3, 4.5e-3 ... 5.7e-3
    cost_bar, coarse_bar, refine_bar = (1e-3, 2e-3, 2e-3) if dtype == torch.float16 else (9e-3, 9e-3, 1.2e-2)
    planes = g["coarse_planes"].tolist()
    check_close(f"coarse cost {dtype}", taps["coarse"]["cost"].float().permute(0, 4, 1, 2, 3)[:, :, planes].cpu(), t(g["coarse_cost"]), rel_l2=cost_bar)
    check_close(f"coarse logits {dtype}", taps["coarse"]["logits"].cpu(), t(g["coarse_logits"]), rel_l2=coarse_bar)
    for i, lt in enumerate(taps["refine"], start=1):
        check_close(f"refine{i} hypotheses {dtype}", lt["hypos"].cpu(), t(g[f"refine{i}_hypos"]), max_abs=0.02 if dtype == torch.float16 else 0.1)
        check_close(f"refine{i} logits {dtype}", lt["logits"].cpu(), t(g[f"refine{i}_logits"]), rel_l2=refine_bar)
    # fp16: the north-star bar.  bf16: at most 15 % above what the storage format itself costs -- the fp32 oracle with every
    # HBM-resident tensor rounded to bf16 (oracle.cvpmvsnet.storage), computed here on the same inputs.
    if dtype == torch.float16:
        dtols = [1e-3] * nscale
    else:
        from oracle import cvpmvsnet as OC
        from test_oracle_cvp import cvp_template
        with torch.no_grad(), OC.storage(dtype):
            emul = OC.forward(scene["imgs"], scene["K"], scene["R"], scene["t"], scene["depth_min"], scene["depth_max"],
                              cvp_weights(g, cvp_template(), seed), nscale=nscale)["depth_est_list"]
        e_emul = [float((emul[i] - t(g[f"depth_est_{i}"])).abs().mean() / t(g[f"depth_est_{i}"]).abs().mean()) for i in range(nscale)]
        print(f"[parity] cvp {dtype} {feature_engine}: storage-emulated oracle depth rel-L1 per level {['%.3e' % e for e in e_emul]}", flush=True)
        dtols = [1.15 * e + 5e-5 for e in e_emul]
    for i in range(nscale):
        s = check_close(f"depth_est_list[{i}] {dtype}", out["depth_est_list"][i].cpu(), t(g[f"depth_est_{i}"]))
        assert s["rel_l1"] <= dtols[i], (s, dtols[i])
    check_close(f"confidence {dtype}", out["photometric_confidence"].cpu(), t(g["photometric_confidence"]), rel_l1=3e-2)


def test_cvp_function_level_warp_and_proj_cost(env):
    """models.CVP_MVSNet.models.modules.homo_warping / proj_cost drop-ins against the oracle (per-pixel hypotheses)."""
    L, ops, synthetic, Frontend = env
    from oracle import cvpmvsnet as OC
    from wild_deep_mvs_amd.models.CVP_MVSNet.models.modules import homo_warping, proj_cost
    g = load_golden("cvp_tiny.npz")
    scene, nscale, seed = cvp_scene(g)
    pyr = t(g["pyr_l0"])                                       # [V,1,16,H,W]
    B = 1
    row = torch.tensor([0., 0., 0., 1.])
    ref_ex = torch.cat((torch.cat((scene["R"][:, 0], scene["t"][:, 0]), 2), row.view(1, 1, 4).expand(B, 1, 4)), 1)
    src_ex = torch.cat((torch.cat((scene["R"][:, 1:], scene["t"][:, 1:]), 3), row.view(1, 1, 1, 4).expand(B, 2, 1, 4)), 2)
    hyp = t(g["refine1_hypos"])
    K = scene["K"]
    want = OC.homo_warping(pyr[1], K[:, 0], K[:, 1], ref_ex, src_ex[:, 0], hyp, pyr[0].shape[2:])
    got = homo_warping(pyr[1].cuda(), K[:, 0].cuda(), K[:, 1].cuda(), ref_ex.cuda(), src_ex[:, 0].cuda(), hyp.cuda(), pyr[0].shape[2:])
    check_close("cvp homo_warping per-pixel", got.cpu(), want, max_abs=3e-4)
    cost = proj_cost(2, pyr[0].cuda(), [[pyr[1].cuda()], [pyr[2].cuda()]], 0, K[:, 0].cuda(), K[:, 1:].cuda(), ref_ex.cuda(),
                     src_ex.cuda(), hyp.cuda(), storage_dtype=torch.float16)
    check_close("cvp proj_cost vs reference golden", cost.float().permute(0, 4, 1, 2, 3).cpu(), t(g["refine1_cost"]), rel_l2=2e-3)


@pytest.mark.parametrize("case", ["scene", "degenerate", "partly_invalid"])
def test_cal_depth_hypo_kernel_vs_oracle(env, case):
    """pscv_cvp_depth_hypos (per-pixel fp64 steps, exact radix-select median, planes; no host round trip) against the
    oracle's restatement of calDepthHypo (modules.py:131-226; pinned to the reference by tests/test_oracle_cvp.py): batch of
    two with different source cameras, the all-invalid fallback (identical cameras: zero epipolar motion) and a map where
    part of the pixels project behind the source camera."""
    L, ops, synthetic, Frontend = env
    from oracle import cvpmvsnet as OC
    from wild_deep_mvs_amd.models.CVP_MVSNet.models.modules import calDepthHypo
    B, V, H, W = (1 if case == "degenerate" else 2), 3, 48, 64   # (the reference's fallback expression only broadcasts for B = 1)
    scene = synthetic.make_scene(B, V, H, W, seed=4)
    scene["t"] = scene["t"] * 8
    scene["t"][B - 1] *= 0.5                                     # a different baseline in the last batch item
    row = torch.tensor([0., 0., 0., 1.])
    ref_ex = torch.cat((torch.cat((scene["R"][:, 0], scene["t"][:, 0]), 2), row.view(1, 1, 4).expand(B, 1, 4)), 1)
    src_ex = torch.cat((torch.cat((scene["R"][:, 1:], scene["t"][:, 1:]), 3), row.view(1, 1, 1, 4).expand(B, V - 1, 1, 4)), 2)
    K = scene["K"]
    gen = torch.Generator().manual_seed(8)
    depth = 2.5 + 3.0 * torch.rand(B, H, W, generator=gen)
    if case == "degenerate":
        src_ex = ref_ex.unsqueeze(1).repeat(1, V - 1, 1, 1)
    if case == "partly_invalid":
        src_ex[:, 0, 2, 3] -= 4.0                                # pushes the nearer half of the depth range behind the source camera
    dmin, dmax = scene["depth_min"][:, 0], scene["depth_max"][:, 0]
    want = OC.cal_depth_hypo(depth, K[:, 0], K[:, 1:], ref_ex, src_ex, dmin, dmax)
    got = calDepthHypo(depth.cuda(), K[:, 0].cuda(), K[:, 1:].cuda(), ref_ex.cuda(), src_ex.cuda(), dmin.cuda(), dmax.cuda(), 0)
    step_want = (want[:, 5] - want[:, 4]).reshape(B, -1)[:, 0]
    print(f"[cal_depth_hypo] {case}: steps {step_want.tolist()}")
    check_close(f"calDepthHypo {case}", got.cpu(), want, max_abs=2e-6)
    # the median itself and every plane against the float64 reference (tests/_depth_hypo_ref.py), constants built on the host
    import numpy as np
    import _depth_hypo_ref as DR
    d_np, cams, fb = DR.inputs({"depth": depth, "ref_in": K[:, 0], "src_in": K[:, 1:], "ref_ex": ref_ex, "src_ex": src_ex, "dmin": dmin, "dmax": dmax})
    hyp, steps = ops.cvp_depth_hypos(depth.cuda(), torch.from_numpy(cams).cuda(), torch.from_numpy(fb).cuda(), want_steps=True)
    r = DR.reference(d_np, cams, fb)
    worst = DR.check_steps(f"calDepthHypo {case}", steps.cpu().numpy(), r)
    print(f"[parity] calDepthHypo {case}: n_valid {r['n_valid'].tolist()}, step distance {worst:.3f} of the bar {DR.STEP_BAR:.2e}", flush=True)
    DR.check_planes(f"calDepthHypo {case}", hyp.cpu().numpy(), r)


def test_cvp_cams_one_launch_equals_tensor_level_camera_algebra(env):
    """pscv_cvp_cams (every per-level camera block of a forward in one launch) against the tensor-level drop-ins it replaces in
    the model's forward: conditionIntrinsics + the projection stack of proj_cost (modules.py:31-50, 89-98) for the warp blocks,
    and the fp64 constants of calDepthHypo (modules.py:131-226) -- batch of two, three source views, a non-power-of-two level."""
    L, ops, synthetic, Frontend = env
    from wild_deep_mvs_amd.models.CVP_MVSNet.models.modules import conditionIntrinsics, _cams, hypo_cams
    B, V, H, W = 2, 4, 96, 120
    scene = synthetic.make_scene(B, V, H, W, seed=11)
    scene["t"][1] *= 0.5
    row = torch.tensor([0., 0., 0., 1.])
    ref_ex = torch.cat((torch.cat((scene["R"][:, 0], scene["t"][:, 0]), 2), row.view(1, 1, 4).expand(B, 1, 4)), 1).cuda()
    src_ex = torch.cat((torch.cat((scene["R"][:, 1:], scene["t"][:, 1:]), 3), row.view(1, 1, 1, 4).expand(B, V - 1, 1, 4)), 2).cuda()
    K = scene["K"].cuda()
    heights = [96, 48, 32, 12]                                   # 96 / 32 = 3: the scaling multiplies by an inexact fp32 reciprocal
    shapes = [(B, 16, h, h * W // H) for h in heights]
    warp, hypo = ops.cvp_cams(K[:, 0], K[:, 1:], ref_ex, src_ex, [H / h for h in heights])
    assert tuple(warp.shape) == (len(heights), V - 1, B, L.CAM_FLOATS) and tuple(hypo.shape) == (len(heights), B, 39)
    ref_ms = conditionIntrinsics(K[:, 0], (B, 3, H, W), shapes)
    src_ms = torch.stack([conditionIntrinsics(K[:, 1 + i], (B, 3, H, W), shapes) for i in range(V - 1)]).permute(1, 0, 2, 3, 4)
    for lv in range(len(heights)):
        want = _cams(ref_ms[:, lv], [src_ms[:, i, lv] for i in range(V - 1)], ref_ex, [src_ex[:, i] for i in range(V - 1)])
        # fp32 projections in both; the 3x3 products may contract in a different order (one fp32 ulp of the entries)
        check_close(f"cvp_cams warp level {lv}", warp[lv].cpu(), want.cpu(), rel_l2=2e-6)
        hw = hypo_cams(ref_ms[:, lv], src_ms[:, 0, lv], ref_ex, src_ex[:, 0])
        rel = float((hypo[lv] - hw).norm() / hw.norm())          # fp64 on both sides
        print(f"[parity] cvp_cams hypo level {lv}: rel_l2={rel:.3e}")
        assert rel <= 1e-12, rel


def test_cvp_graphed_forward_replays_equal_eager(env):
    """graph.GraphedModel on the CVP-MVSNet mirror: the capture and FOUR replays return the eager result bit for bit.  The radix
    select of pscv_cvp_depth_hypos used to clear its histograms with a hipMemsetAsync node, which a replayed hipGraph did not
    re-execute correctly (first replay right, later ones with the previous counters: refinement depths off by 0.3)."""
    L, ops, synthetic, Frontend = env
    from wild_deep_mvs_amd.graph import GraphedModel
    g = load_golden("cvp_tiny.npz")
    scene, nscale, seed = cvp_scene(g)
    net = Frontend()
    net.load_state_dict(synthetic.sharpened_state_dict("cvp", synthetic.template_of(net), seed=seed), strict=True)
    net = net.cuda().eval()
    dev = {k: v.cuda() for k, v in scene.items()}
    a = (dev["imgs"], dev["K"], dev["R"], dev["t"], dev["depth_min"], dev["depth_max"])
    want = net(*a, nscale=nscale)
    gnet = GraphedModel(net)
    for r in range(5):
        got = gnet(*a, nscale=nscale)
        for i in range(nscale):
            assert torch.equal(got["depth_est_list"][i], want["depth_est_list"][i]), (r, i)
    assert len(gnet._graphs) == 1


def test_cvp_list_input_and_reference_frame(env):
    """List input (test-mode loaders) and reference_frame != 0 through the CVP mirror (frontend.py:10-38), against the oracle."""
    L, ops, synthetic, Frontend = env
    from oracle import cvpmvsnet as OC
    g = load_golden("cvp_tiny.npz")
    scene, nscale, seed = cvp_scene(g)
    net = Frontend()
    sd = synthetic.sharpened_state_dict("cvp", synthetic.template_of(net), seed=seed)
    net.load_state_dict(sd, strict=True)
    net = net.cuda().eval()
    dev = {k: v.cuda() for k, v in scene.items()}
    V = scene["imgs"].shape[1]
    with torch.no_grad():
        out = net([dev["imgs"][:, i] for i in range(V)], dev["K"], dev["R"], dev["t"], dev["depth_min"], dev["depth_max"],
                  reference_frame=1, nscale=nscale)
        ref = OC.forward(scene["imgs"], scene["K"], scene["R"], scene["t"], scene["depth_min"], scene["depth_max"], sd, nscale=nscale,
                         reference_frame=1)
    s = check_close("cvp reference_frame=1 depth vs oracle", out["depth"].cpu(), ref["depth"])
    assert s["rel_l1"] <= 1e-3, s
    s = check_close("cvp reference_frame=1 depth vs the reference's own output", out["depth"].cpu(), t(load_golden("refframe_tiny.npz")["cvp_depth"]))
    assert s["rel_l1"] <= 1e-3, s
