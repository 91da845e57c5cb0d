"""End-to-end: the MVSNet mirror on the HIP engine vs the reference goldens / the oracle."""
import numpy as np
import pytest
import torch

from _util import bf16_round, check_close, golden_rig, load_golden, t

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from wild_deep_mvs_amd import _lib as L, ops, synthetic
    from wild_deep_mvs_amd.models.MVSNet.model import MVSNet
    from oracle import mvsnet as O
    return L, ops, synthetic, MVSNet, O


def _model(env, agg, seed, dtype=torch.float16):
    L, ops, synthetic, MVSNet, O = env
    net = MVSNet(agg)
    sd = synthetic.sharpened_state_dict("mvsnet", synthetic.template_of(net), seed=seed)
    net.load_state_dict(sd, strict=True)
    net.storage_dtype = dtype
    return net.cuda().eval(), sd


# Depth tolerance per storage format.  fp16 storage (the default) meets the north-star 1e-3 relative L1 with ~5x margin.
# bf16 storage carries an 8-bit significand through 13 stored tensors; on these deliberately unsaturated softmaxes (mean
# max-prob 0.2-0.8) the IDEAL bf16 pipeline -- the fp32 oracle with every stored tensor rounded to bf16, DESIGN.md section 3 --
# already sits at 0.8-1.3e-3.  So the bf16 bar is NOT a loose constant: the engine may exceed the error of that storage-emulated
# oracle (computed in the test, same inputs) by at most 15 %, which a kernel regression cannot hide under.
DEPTH_TOL = {torch.float16: 1e-3}
EMUL_SLACK = 1.15


def emulated_depth_error(O, scene, sd, D, agg, dtype, ref_depth, feature_layers):
    """relative L1 of the storage-emulated oracle (fp32 arithmetic, every HBM-resident tensor rounded to `dtype`) against the
    reference golden: what an ideal pipeline with this storage format does."""
    with torch.no_grad():
        emul = O.forward(scene["imgs"], scene["K"], scene["R"], scene["t"], scene["depth_min"], scene["depth_max"], sd,
                         num_depth=D, aggregation=agg, store=dtype, store_feature_layers=feature_layers)["depth"]
    return float((emul - ref_depth).abs().mean() / ref_depth.abs().mean())


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_cost_reg_net_layers_vs_oracle(env, dtype):
    """Every stored stage of the 3-D U-Net against the oracle run on the same (16-bit rounded) cost volume."""
    L, ops, synthetic, MVSNet, O = env
    g = load_golden("mvsnet_tiny.npz")
    net, sd = _model(env, "variance", int(g["meta"][4]), dtype)
    cost = t(g["cost_volume"]).to(dtype).float()
    taps_ref, taps = {}, {}
    with torch.no_grad():
        ref_logits = O.cost_reg_net(cost, sd, taps=taps_ref).squeeze(1)
        logits = net.cost_regularization(ops.to_channels_last(cost.cuda(), dtype), taps)
    tol = 1e-2 if dtype == torch.bfloat16 else 1.5e-3
    for k in ("conv0", "conv2", "conv4", "conv6", "up7", "up9", "up11"):
        check_close(f"reg {k} {dtype}", taps[k].float().permute(0, 4, 1, 2, 3).cpu(), taps_ref[k], rel_l2=tol)
    check_close(f"reg logits {dtype}", logits.cpu(), ref_logits, rel_l2=tol)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_feature_net_engine_vs_reference_features(env, dtype):
    """The 2-D extractor as eight MFMA conv2d launches (16-bit activations between the layers, BatchNorm folded)
    against the reference's fp32 feature maps (golden), next to the PyTorch-ROCm path rounded once at the end."""
    L, ops, synthetic, MVSNet, O = env
    g = load_golden("mvsnet_tiny.npz")
    H, W, V, D, seed, scene_seed, behind = [int(x) for x in g["meta"]]
    net, sd = _model(env, "variance", seed, dtype)
    scene = synthetic.make_scene(1, V, H, W, seed=scene_seed, behind_view=behind)
    imgs = [scene["imgs"][:, v].cuda() for v in range(V)]
    ref = t(g["features"])                                                   # [V,1,32,h,w]
    with torch.no_grad():
        net.feature_engine = "pscv"
        got = torch.stack([f.float().permute(0, 3, 1, 2).cpu() for f in net.extract_features_cl(imgs)])
        net.feature_engine = "torch"
        base = torch.stack([f.float().permute(0, 3, 1, 2).cpu() for f in net.extract_features_cl(imgs)])
    ulp = 2 ** -8 if dtype == torch.bfloat16 else 2 ** -11
    check_close(f"torch features rounded to {dtype}", base, ref, rel_l2=ulp)
    # eight stored layers instead of one final rounding: a few ulp of relative L2
    check_close(f"pscv conv2d features {dtype}", got, ref, rel_l2=6 * ulp)
    assert got.shape == ref.shape


@pytest.mark.parametrize("feature_engine", ["pscv", "torch"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("fname,agg", [("mvsnet_tiny.npz", "variance"), ("mvsnet_behind.npz", "variance"),
                                        ("mvsnet_dtu_tiny.npz", "variance"), ("mvsnet_s_tiny.npz", "softmin")])
def test_forward_depth_parity_with_reference(env, fname, agg, dtype, feature_engine):
    """forward(imgs, K, R, t, depth_min, depth_max) -> depth within 1e-3 relative L1 of the reference's
    fp32 PyTorch path (BASELINE.json north_star) with fp16 storage / fp32 accumulation (see DEPTH_TOL for bf16),
    with the 2-D extractor on the HIP engine (default) and on PyTorch-ROCm."""
    L, ops, synthetic, MVSNet, O = env
    g = load_golden(fname)
    H, W, V, D, seed, scene_seed, behind = [int(x) for x in g["meta"]]
    net, sd = _model(env, agg, seed, dtype)
    net.feature_engine = feature_engine
    net.num_depth = D
    scene = synthetic.make_scene(1, V, H, W, seed=scene_seed, behind_view=behind, rig=golden_rig(g))
    dev = {k: v.cuda() for k, v in scene.items()}
    taps = {}
    out = net(dev["imgs"], dev["K"], dev["R"], dev["t"], dev["depth_min"], dev["depth_max"], taps=taps)
    assert set(out) == {"depth", "depth_est_list", "depth_pair_list", "photometric_confidence"}
    assert tuple(out["depth"].shape) == (1, H // 4, W // 4) and out["depth_pair_list"] == []
    # Intermediate tensors, bars per storage format at ~2 x the values measured in round 6 (one bar of 1e-2 / 3e-2 for everything
    # before): fp16 cost volume 3.4e-4 ... 1.3e-3, logits 3.4e-4 ... 7.4e-4; bf16 cost volume 2.8e-3 ... 6.4e-3 with the PyTorch-ROCm
    # extractor and 6.5e-3 ... 1.05e-2 with the engine's (bf16 activations through its eight 2-D layers), logits 3.6e-3 ... 6.0e-3.
    if dtype == torch.float16:
        cv_bar, lg_bar = 2.5e-3, 1.5e-3
    else:
        cv_bar, lg_bar = (2e-2 if feature_engine == "pscv" else 1.2e-2), 1.2e-2
    check_close(f"{fname} cost volume ({dtype})", taps["cost_volume"].float().permute(0, 4, 1, 2, 3).cpu(), t(g["cost_volume"]),
                rel_l2=cv_bar)
    check_close(f"{fname} logits ({dtype})", taps["logits"].cpu(), t(g["logits"]).squeeze(1), rel_l2=lg_bar)
    ref = t(g["depth"])
    s = check_close(f"{fname} depth ({dtype})", out["depth"].cpu(), ref)
    if dtype in DEPTH_TOL:
        assert s["rel_l1"] <= DEPTH_TOL[dtype], s
    else:
        e_emul = emulated_depth_error(O, scene, sd, D, agg, dtype, ref, feature_layers=feature_engine == "pscv")
        print(f"[parity] {fname} {dtype} {feature_engine}: engine {s['rel_l1']:.3e} vs storage-emulated oracle {e_emul:.3e}", flush=True)
        assert s["rel_l1"] <= EMUL_SLACK * e_emul + 2e-5, (s, e_emul)
    # the confidence window is anchored at trunc(E[index]) (model.py:213), so it jumps where E[index] crosses an
    # integer: compare in the mean, and point-wise only away from those crossings
    conf, conf_ref = out["photometric_confidence"].cpu(), t(g["photometric_confidence"])
    check_close(f"{fname} confidence ({dtype})", conf, conf_ref, rel_l1=2e-2)
    prob = torch.softmax(t(g["logits"]).squeeze(1), 1)
    eidx = (prob * torch.arange(D, dtype=torch.float32).view(1, D, 1, 1)).sum(1)
    stable = (eidx - eidx.round()).abs() > 0.05
    assert float((conf - conf_ref)[stable].abs().max()) <= 0.05
    # the reference's own evaluation quantity: error in units of (max-min)/128 (depthmap_eval.py:133-143)
    unit = (float(scene["depth_max"][0, 0]) - float(scene["depth_min"][0, 0])) / 128
    epe = float((out["depth"].cpu() - ref).abs().mean()) / unit
    print(f"[parity] {fname} {dtype} EPE vs reference = {epe:.4f} depth units", flush=True)
    assert epe < (0.05 if dtype == torch.float16 else 0.3)


def test_list_input_and_reference_frame(env):
    """imgs may be a list of V tensors (test-mode loaders) and any view can be the reference."""
    L, ops, synthetic, MVSNet, O = env
    net, sd = _model(env, "variance", 0)
    net.num_depth = 16
    scene = synthetic.make_scene(1, 3, 64, 96, seed=2)
    dev = {k: v.cuda() for k, v in scene.items()}
    out = net(list(torch.unbind(dev["imgs"], 1)), dev["K"], dev["R"], dev["t"], dev["depth_min"], dev["depth_max"],
              reference_frame=1)
    with torch.no_grad():
        ref = O.forward(scene["imgs"], scene["K"], scene["R"], scene["t"], scene["depth_min"], scene["depth_max"], sd,
                        num_depth=16, reference_frame=1)
    s = check_close("reference_frame=1 depth", out["depth"].cpu(), ref["depth"])
    assert s["rel_l1"] <= 1e-3
    # ... and against the depth map the REFERENCE produced for this call shape (tests/golden/gen_golden.py --only refframe: scene seed 0)
    scene0 = {k: v.cuda() for k, v in synthetic.make_scene(1, 3, 64, 96, seed=0).items()}
    out0 = net(list(torch.unbind(scene0["imgs"], 1)), scene0["K"], scene0["R"], scene0["t"], scene0["depth_min"], scene0["depth_max"],
               reference_frame=1)
    s = check_close("reference_frame=1 depth vs the reference's own output", out0["depth"].cpu(), t(load_golden("refframe_tiny.npz")["mvsnet_depth"]))
    assert s["rel_l1"] <= 1e-3


def test_training_mode_runs_on_the_engine(env):
    """train() mode is the engine's autograd path (tests/test_gpu_train.py holds its parity); the eval-only entry point of
    the U-Net refuses to be called in train() mode instead of silently folding stale running statistics."""
    L, ops, synthetic, MVSNet, O = env
    net, _ = _model(env, "variance", 0)
    net.train()
    scene = {k: v.cuda() for k, v in synthetic.make_scene(1, 3, 64, 96).items()}
    out = net(scene["imgs"], scene["K"], scene["R"], scene["t"], scene["depth_min"], scene["depth_max"])
    assert out["depth"].requires_grad
    with pytest.raises(RuntimeError):
        net.cost_regularization(torch.zeros(1, 16, 16, 24, 32, dtype=torch.float16, device="cuda"))


def test_invalidate_after_a_write_through_dot_data(env):
    """The packed-weight caches key on (address, tensor._version).  A write through ``.data`` does not bump the version, so the
    engine keeps the packed copy until ``wild_deep_mvs_amd.invalidate()`` is called (documented in ops.invalidate_weight_caches);
    in-place ops on the Parameter itself are picked up without it."""
    import wild_deep_mvs_amd
    L, ops, synthetic, MVSNet, O = env
    net, sd = _model(env, "variance", 0)
    net.num_depth = 16
    scene = synthetic.make_scene(1, 3, 64, 96, seed=2)
    dev = {k: v.cuda() for k, v in scene.items()}
    run = lambda: net(dev["imgs"], dev["K"], dev["R"], dev["t"], dev["depth_min"], dev["depth_max"])["depth"].clone()
    d0 = run()
    w = net.cost_regularization.prob.weight
    v0 = w._version
    w.data.mul_(-1.0)                                   # flips the sign of every logit: the soft-argmin must change
    assert w._version == v0                             # ... but the version counter did not move
    assert torch.equal(run(), d0)                       # stale packed weights: the documented hazard
    wild_deep_mvs_amd.invalidate()
    d1 = run()
    assert float((d1 - d0).abs().mean()) > 1e-3 * float(d0.abs().mean())
    with torch.no_grad():
        w.mul_(-1.0)                                    # in-place op on the Parameter: version bump, no invalidate needed
    assert torch.equal(run(), d0)


def test_fused_tail_option_equals_default_path(env):
    """models.MVSNet.model.FUSED_TAIL (prob head + softmax regression through pscv_prob_softargmin; off by default because it measured
    slower) gives the depth and confidence of the default path on a full forward."""
    L, ops, synthetic, MVSNet, O = env
    from wild_deep_mvs_amd.models.MVSNet import model as M
    net, sd = _model(env, "variance", 0)
    net.num_depth = 48
    scene = synthetic.make_scene(1, 3, 64, 96, seed=2)
    dev = {k: v.cuda() for k, v in scene.items()}
    run = lambda: net(dev["imgs"], dev["K"], dev["R"], dev["t"], dev["depth_min"], dev["depth_max"])
    want = run()
    M.FUSED_TAIL = True
    try:
        with L.tuning(c1_sweep=2):
            got = run()
    finally:
        M.FUSED_TAIL = False
    check_close("fused tail depth", got["depth"].cpu(), want["depth"].cpu(), max_abs=2e-5)
    check_close("fused tail confidence", got["photometric_confidence"].cpu(), want["photometric_confidence"].cpu(), max_abs=5e-5)


def test_stream_mode_equals_the_sequential_forward_at_the_headline_size(env):
    """Three reference views of 5 x 512x640, D = 192 on three HIP streams: here one view's warp really overlaps another view's
    conv kernels for ~100 us at a time, the condition under which the LDS-staged warp kernel was found NOT reproducible at the
    end of round 3 (39 of 40 such steps differed from the sequential forward by up to 8e-2 of the depth range; DESIGN.md
    section 6).  Since round 4 the kernel ships as its scalar-fp32 build, so with
    DEFAULT tuning every step equals the one-stream forward bit for bit."""
    L, ops, synthetic, MVSNet, O = env
    net = MVSNet("variance")
    net.load_state_dict(synthetic.sharpened_state_dict("mvsnet", synthetic.template_of(net), seed=0))
    net = net.cuda().eval()
    net.num_depth, net.graph_replay = 192, False
    sc = {k: v.cuda() for k, v in synthetic.make_scene(3, 5, 512, 640, seed=7).items()}
    call = lambda: net(sc["imgs"], sc["K"], sc["R"], sc["t"], sc["depth_min"], sc["depth_max"])
    with torch.no_grad():
        assert net.batch_streams is False, "one stream is the default"
        assert L.get_tuning("warp_tiled") == 1, "default tuning"
        ref = call()
        net.batch_streams = True
        for rep in range(12):
            got = call()
            assert torch.equal(got["depth"], ref["depth"]) and torch.equal(got["photometric_confidence"], ref["photometric_confidence"]), rep
    assert L.get_tuning("warp_tiled") == 1, "default tuning throughout"


@pytest.mark.parametrize("B", [2, 3])
def test_batch_items_on_separate_streams_equal_the_one_item_runs(env, B):
    """``MVSNet._hot_path_streams``: the reference views of a batch run on their own HIP streams (one item's VALU-bound warp
    beside another's MFMA / memory-bound U-Net), eager launches only.  The inputs CHANGE from call to call (a stale read or a
    race between the streams must show): depth and confidence equal the one-item runs bit for bit on every one of eight
    calls, and the stream-less batched launches (``batch_streams = False``) to fp32 order.  Under a hipGraph capture the fork
    becomes parallel branches of the graph (``batch_streams_capture``, default since round 4): six replays on CHANGING inputs equal
    the one-item runs bit for bit -- round 3 saw such graphs replay wrongly; the cause was the packed warp build's overlap defect
     -- and with ``batch_streams_capture = False`` the captured forward does not fork and equals the batched run."""
    L, ops, synthetic, MVSNet, O = env
    net = MVSNet("variance")
    net.load_state_dict(synthetic.sharpened_state_dict("mvsnet", synthetic.template_of(net), seed=0))
    net = net.cuda().eval()
    net.num_depth, net.graph_replay = 32, False
    net.batch_streams = True          # (opt-in: a caller's batch otherwise runs as one launch per layer on the caller's stream)
    keys = ("imgs", "K", "R", "t", "depth_min", "depth_max")

    def batch_of(seed0):
        scenes = [synthetic.make_scene(1, 4, 128, 160, seed=seed0 + b) for b in range(B)]
        return scenes, {k: torch.cat([sc[k] for sc in scenes], 0).cuda() for k in keys}
    with torch.no_grad():
        for it in range(8):
            scenes, batch = batch_of(20 + 7 * it)
            got = net(*[batch[k] for k in keys])
            net.batch_streams = False
            singles = [net(*[sc[k].cuda() for k in keys]) for sc in scenes]
            plain = net(*[batch[k] for k in keys])
            net.batch_streams = True
            for b in range(B):
                assert torch.equal(got["depth"][b], singles[b]["depth"][0]), (it, b)
                assert torch.equal(got["photometric_confidence"][b], singles[b]["photometric_confidence"][0]), (it, b)
            assert float((plain["depth"] - got["depth"]).abs().max()) <= 1e-5 * float(got["depth"].abs().max())
        for fork in (True, False):
            # captured: the fork is part of the graph (or, fork = False, the plain batched launches); replays on changing inputs are right
            net.batch_streams_capture = fork
            scenes, batch = batch_of(100)
            static = {k: batch[k].clone() for k in keys}
            for _ in range(2):
                net(*[static[k] for k in keys])
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                out = net(*[static[k] for k in keys])
            for rep in range(6):
                scenes, batch = batch_of(200 + 5 * rep)
                for k in keys:
                    static[k].copy_(batch[k])
                g.replay()
                torch.cuda.synchronize()
                net.batch_streams = False
                if fork:
                    singles = [net(*[sc[k].cuda() for k in keys]) for sc in scenes]
                    ok = all(torch.equal(out["depth"][b], singles[b]["depth"][0]) and
                             torch.equal(out["photometric_confidence"][b], singles[b]["photometric_confidence"][0]) for b in range(B))
                else:
                    want = net(*[batch[k] for k in keys])
                    ok = torch.equal(out["depth"], want["depth"]) and torch.equal(out["photometric_confidence"], want["photometric_confidence"])
                net.batch_streams = True
                assert ok, (fork, rep)
        net.batch_streams_capture = True


@pytest.mark.parametrize("B,size", [(3, (128, 160, 32)), (3, (512, 640, 192))])
def test_view_pipeline_free_running_steps_equal_the_one_item_runs(env, B, size):
    """``graph.ViewPipeline`` (round 6: bench.py's step): one single-branch hipGraph per reference view, each replayed on its own HIP
    stream, consecutive steps NOT joined.  Several steps are launched back to back without a host wait, the inputs are rewritten
    (after ``results()`` has joined the streams) between rounds: depth and confidence of the last step equal eager one-item launches on
    one stream bit for bit -- at a small size and at the headline size, where one view's warp really runs beside another view's U-Net."""
    L, ops, synthetic, MVSNet, O = env
    from wild_deep_mvs_amd.graph import ViewPipeline
    from wild_deep_mvs_amd.models.MVSNet.model import build_proj_matrices
    H, W, D = size
    net = MVSNet("variance")
    net.load_state_dict(synthetic.sharpened_state_dict("mvsnet", synthetic.template_of(net), seed=0))
    net = net.cuda().eval()
    net.num_depth, net.graph_replay = D, False
    V, C, h, w = 5, 32, H // 4, W // 4
    cams = synthetic.make_cameras(B, V, H, W)
    Ks = cams["K"].clone()
    Ks[:, :, :2] /= 4
    proj = build_proj_matrices(Ks, cams["R"], cams["t"]).cuda()
    steps = torch.arange(D, dtype=torch.float32).view(1, -1)
    dv = (cams["depth_min"][:, :1] + (cams["depth_max"][:, :1] - cams["depth_min"][:, :1]) / (D - 1) * steps).cuda().contiguous()
    feats = synthetic.make_features(B, V, C, h, w, seed=3)
    fcl = [ops.to_channels_last(feats[i].cuda(), torch.bfloat16) for i in range(V)]
    net.storage_dtype = torch.bfloat16
    with torch.no_grad():
        pipe = ViewPipeline(net, fcl, proj, dv)
        for rnd in range(4):
            for f in fcl:                                            # new inputs, in place (the graphs read the live tensors)
                f.copy_(torch.roll(f, shifts=(1 + rnd, 2), dims=(1, 2)))
            for _ in range(1 + 2 * rnd):                             # 1, 3, 5, 7 un-joined steps
                pipe.step()
            depth, conf = pipe.results()
            torch.cuda.synchronize()
            for b in range(B):
                d1, c1 = net.hot_path([f[b:b + 1] for f in fcl], proj[b:b + 1], dv[b:b + 1])
                assert torch.equal(depth[b], d1[0]) and torch.equal(conf[b], c1[0]), (rnd, b)
