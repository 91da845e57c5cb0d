"""GPU: the loss reductions and depth-map scores of csrc/depth_gt.hip against the fixture
tests/golden/gtloss_tiny.npz and the restatement tests/_gt_loss_ref.py, and ``Trainer.step`` / ``Trainer.test`` with
``loss_engine = "pscv"`` against the torch path on the same weights."""
import os
import types

import numpy as np
import pytest
import torch

from tests import _gt_loss_ref as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gtloss_tiny.npz")


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from wild_deep_mvs_amd import _lib as L, ops, training as T
    with np.load(GOLDEN) as f:
        z = {k: f[k] for k in f.files}
    return types.SimpleNamespace(L=L, ops=ops, T=T, z=z, terms=R.fixture_terms(z))


def _cuda(x, grad=False):
    if x is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    return t.requires_grad_() if grad else t


def _table(env, terms, grad=False):
    return [env.ops.LossTerm(t["kind"], t["factor"], _cuda(t["a"], grad), _cuda(t["mask"]), _cuda(t["u"], grad), _cuda(t["gt"]),
                             _cuda(t["interval"])) for t in terms]


@pytest.fixture(scope="module")
def run(env):
    """One forward + backward of the whole fixture table through the autograd node (shared, not modified by the tests)."""
    table = _table(env, env.terms, grad=True)
    loss, term, sums = env.T.loss_terms(table)
    g_up = 0.7
    (loss * g_up).backward()
    torch.cuda.synchronize()
    return types.SimpleNamespace(table=table, loss=loss.detach().cpu(), term=term.cpu().numpy(), sums=sums.cpu().numpy(), g_up=g_up)


def test_all_four_kinds_in_one_table_against_the_fixture(env, run):
    want = np.array([t["want"] for t in env.terms])
    want_loss = float(sum(t["factor"] * t["want"] for t in env.terms))
    print("loss", float(run.loss), want_loss, "max term err", np.abs(run.term - want).max())
    assert run.term.shape == (20,) and run.sums.shape == (20, 3) and run.sums.dtype == np.float64
    assert np.all(np.abs(run.term - want) <= 1e-5 * np.maximum(1.0, np.abs(want)))
    assert abs(float(run.loss) - want_loss) <= 1e-5 * max(1.0, abs(want_loss))
    counts = np.array([R.term_of(t)["sums"][2] for t in env.terms])
    assert np.array_equal(run.sums[:, 2], counts) and counts[-1] == 0 and counts[0] == float(env.z["s1_count"])
    for i, t in enumerate(env.terms):
        ref = R.term_of(t)["sums"]
        assert abs(run.sums[i, 0] - ref[0]) <= 1e-5 * max(1.0, abs(ref[0])) and abs(run.sums[i, 1] - ref[1]) <= 1e-5 * max(1.0, abs(ref[1])), i


def test_gradients_against_the_restatement_and_exact_zeros_under_the_mask(env, run):
    for i, (t, row) in enumerate(zip(env.terms, run.table)):
        da, du = R.grads_of(t, run.g_up)
        valid = R.pixel_loss(t["kind"], t["a"], t["gt"], t["mask"], t["interval"])[1].reshape(da.shape)
        got = row.a.grad.cpu().numpy().astype(np.float64)
        assert got.shape == da.shape and np.all(np.abs(got - da) <= 1e-5 * np.abs(da) + 1e-7), (i, np.abs(got - da).max())
        assert np.all(got[~valid] == 0) and (~valid).any()
        if du is None:
            assert row.u is None
        else:
            gu = row.u.grad.cpu().numpy().astype(np.float64)
            assert np.all(np.abs(gu - du) <= 1e-5 * np.abs(du) + 1e-7), (i, np.abs(gu - du).max())
            assert np.all(gu[~valid.reshape(gu.shape)] == 0)
    s1 = run.table[0].a.grad.cpu().numpy()
    assert np.all(s1[:, 1, 2] == 0)                                  # d == gt_down: sign(0) = 0


def test_a_second_call_gives_identical_bits(env, run):
    table = _table(env, env.terms, grad=True)
    loss, term, sums = env.T.loss_terms(table)
    (loss * run.g_up).backward()
    assert loss.detach().cpu().numpy().tobytes() == run.loss.numpy().tobytes()
    assert sums.cpu().numpy().tobytes() == run.sums.tobytes() and term.cpu().numpy().tobytes() == run.term.tobytes()
    for a, b in zip(table, run.table):
        assert torch.equal(a.a.grad, b.a.grad) and (a.u is None or torch.equal(a.u.grad, b.u.grad))


def test_unaligned_and_odd_sized_terms_take_the_scalar_path(env):
    """Views that start 4 bytes into an allocation and a pixel count that is no multiple of four: no 16-byte accesses."""
    rng = np.random.default_rng(5)
    n = 1027
    l, u, m = rng.random(n + 1).astype(np.float32), rng.normal(0, 0.5, n + 1).astype(np.float32), rng.random(n + 1) > 0.3
    lt, ut, mt = (_cuda(l)[1:].requires_grad_(), _cuda(u)[1:].requires_grad_(), _cuda(m)[1:])
    loss, term, sums = env.T.loss_terms([env.ops.LossTerm(R.L_BAYES, 2.0, lt, mt, u=ut)])
    loss.backward()
    ref = R.term(R.L_BAYES, l[1:], m[1:], u[1:])
    da, du = R.term_grads(R.L_BAYES, 2.0, 1.0, l[1:], m[1:], u[1:])
    assert abs(float(term[0]) - ref["value"]) <= 1e-5 * max(1.0, abs(ref["value"])) and float(sums[0, 2]) == ref["sums"][2]
    assert np.all(np.abs(lt.grad.cpu().numpy() - da) <= 1e-5 * np.abs(da) + 1e-7)
    assert np.all(np.abs(ut.grad.cpu().numpy() - du) <= 1e-5 * np.abs(du) + 1e-7)


def test_empty_masks(env):
    z = env.z
    none = np.zeros_like(z["gt_mask"])
    bayes = env.ops.LossTerm(R.GT_BAYES, 1.0, _cuda(z["s2_p0_d"], True), _cuda(none), _cuda(z["s2_p0_u"], True), _cuda(z["gt"]), _cuda(z["interval"]))
    loss, term, sums = env.T.loss_terms([bayes])
    loss.backward()
    assert float(loss.detach()) == 0.0 and float(sums[0, 2]) == 0.0
    assert torch.count_nonzero(bayes.a.grad) == 0 and torch.count_nonzero(bayes.u.grad) == 0
    plain = env.ops.LossTerm(R.GT_PLAIN, 1.0, _cuda(z["s2_d"]), _cuda(none), gt=_cuda(z["gt"]), interval=_cuda(z["interval"]))
    assert torch.isnan(env.ops.loss_terms([plain])["loss"])


def test_32_terms_in_one_call_and_33_raise(env):
    rows = _table(env, (env.terms * 2)[:32])
    o = env.ops.loss_terms(rows)
    want = np.array([t["want"] for t in (env.terms * 2)[:32]])
    assert np.all(np.abs(o["term"].cpu().numpy() - want) <= 1e-5 * np.maximum(1.0, np.abs(want)))
    with pytest.raises(env.L.PscvError, match="33 terms"):
        env.ops.loss_terms(rows + rows[:1])


def test_forward_and_backward_never_wait_for_the_device(env):
    table = _table(env, env.terms, grad=True)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss, term, sums = env.T.loss_terms(table)
        loss.backward()
        m = env.ops.depth_metrics(table[2].a.detach(), table[0].gt, table[0].mask, table[0].interval)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert torch.isfinite(loss) and torch.isfinite(m["EPE"]) and table[0].a.grad is not None


# ---- scores ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["m4", "m1", "mf"])          # 6x12 (upsampled 4x), 24x48 (identity), 7x13 (a non-integer ratio)
def test_scores_against_the_fixture(env, name):
    z = env.z
    step = (z["m_max"][:, 0] - z["m_min"][:, 0]) / np.float32(128)
    thr, rel = tuple(float(t) for t in z["m_thresholds"]), tuple(float(r) for r in z["m_rel_thresholds"])
    est = z[f"{name}_est"]
    assert R.threshold_margin(est, z["m_gt"], z["m_mask"], step, thr, rel) > 1e-3          # the counts cannot differ by rounding
    for mask in (z["m_mask"], z["m_mask"] > 0.5):                                           # fp32 and bool
        m = env.ops.depth_metrics(_cuda(est), _cuda(z["m_gt"]), _cuda(mask), _cuda(step), thresholds=thr, rel_thresholds=rel)
        sums = m["sums"].cpu().numpy()
        assert np.array_equal(sums[:, 0], z[f"{name}_count"])
        assert np.array_equal(sums[:, 2:4], z[f"{name}_thres_counts"]) and np.array_equal(sums[:, 8:10], z[f"{name}_rel_counts"])
        for key in ("EPE", "Rel", "SqRel"):
            want = float(z[f"{name}_{key}"])
            print(name, key, float(m[key]), want)
            assert abs(float(m[key]) - want) <= 1e-5 * abs(want), (key, float(m[key]), want)
        assert np.allclose(m["thres"].cpu().numpy(), z[f"{name}_thres"], rtol=0, atol=1e-6)
        assert np.allclose(m["rel_thres"].cpu().numpy(), z[f"{name}_rel_thres"], rtol=0, atol=1e-6)
        ref = R.metrics(est, z["m_gt"], z["m_mask"], step, thr, rel)
        assert np.allclose(m["per_image"]["EPE"].cpu().numpy(), ref["per_image"]["EPE"], rtol=1e-5, atol=0)
    if name == "m1":                                                                        # h = H is a copy: no step, |e - g| exact
        m = env.ops.depth_metrics(_cuda(est), _cuda(z["m_gt"]), _cuda(z["m_mask"]), thresholds=())
        want = R.metrics(est, z["m_gt"], z["m_mask"], None, ())
        assert np.allclose(m["sums"].cpu().numpy()[:, 1], want["sums"][:, 1], rtol=1e-12, atol=0)


def test_an_image_with_an_empty_mask_scores_nan(env):
    z = env.z
    mask = z["m_mask"].copy()
    mask[1] = 0
    m = env.ops.depth_metrics(_cuda(z["m4_est"]), _cuda(z["m_gt"]), _cuda(mask), thresholds=(1, 3), rel_thresholds=(1.25,))
    per = m["per_image"]
    assert torch.isfinite(per["EPE"][0]) and torch.isnan(per["EPE"][1]) and torch.isnan(per["thres"][1]).all() and torch.isnan(per["rel_thres"][1]).all()
    assert torch.isnan(m["EPE"]) and float(m["sums"][1, 0]) == 0.0
    with pytest.raises(env.L.PscvError, match="thresholds"):
        env.ops.depth_metrics(_cuda(z["m4_est"]), _cuda(z["m_gt"]), _cuda(mask), rel_thresholds=(1, 2, 3, 4, 5))


# ---- the trainer -----------------------------------------------------------------------------------------------------------------
def _args(**kw):
    base = dict(architecture="mvsnet", upsample_training=False, occ_masking=False, supervised=False, num_im_train=3, print_every=1,
                dataset="dtu_yao", geom_clamping=0.01)
    base.update(kw)
    return types.SimpleNamespace(**base)


def _sample(synthetic, V=3, H=64, W=96, seed=2):
    """The scene of tests/test_gpu_harness.py::_sample."""
    scene = synthetic.make_scene(1, V, H, W, seed=seed)
    depth = (0.5 * (scene["depth_min"][:, :1] + scene["depth_max"][:, :1])).view(1, 1, 1, 1).expand(1, 1, H, W).clone()
    depth = depth * (1.0 + 0.1 * torch.rand(1, 1, H, W, generator=torch.Generator().manual_seed(0)))
    mask = torch.ones(1, 1, H, W)
    mask[..., :4, :] = 0
    return dict(scene, depth=depth, mask=mask)


def _net(kind):
    from wild_deep_mvs_amd import synthetic
    if kind == "mvsnet":
        from wild_deep_mvs_amd.models.MVSNet.model import MVSNet
        net = MVSNet("variance")
        net.load_state_dict(synthetic.sharpened_state_dict("mvsnet", synthetic.template_of(net), seed=0))
        net.num_depth = 16
    else:
        from wild_deep_mvs_amd.models.VisMVSNet.frontend import Frontend
        net = Frontend()
        net.load_state_dict(synthetic.sharpened_state_dict("vis", synthetic.template_of(net), seed=0))
        net.depth_nums, net.interval_scales = [16, 8, 4], [8.0, 4.0, 2.0]          # the sizes of tests/golden/vis_train.npz
    return net.cuda().train()


@pytest.mark.parametrize("architecture,supervised", [("mvsnet", True), ("mvsnet", False), ("vis_mvsnet", True)])
def test_trainer_step_pscv_equals_torch(env, architecture, supervised):
    from wild_deep_mvs_amd import synthetic
    from wild_deep_mvs_amd.models.trainer import Trainer
    net = _net("mvsnet" if architecture == "mvsnet" else "vis")
    # The whole network on the engine, the 2-D extractor included (the default in train() runs it on torch's convolutions): this
    # forward gave the same bits in every run and on every call, so the two steps differ by the loss tail alone.  With the torch
    # extractor the loss of this very step came out as 149.367, 149.444 and 149.476 in runs on three machines, and in a clean
    # checkout as 149.444 and then 149.547 for two consecutive steps of one process: a difference upstream of any loss code,
    # which the 1e-5 below would charge to the loss engines.
    net.feature_engine_train = "pscv"
    sample = _sample(synthetic)
    out = {}
    for engine in ("torch", "pscv"):
        tr = Trainer(net, _args(architecture=architecture, supervised=supervised))
        tr.loss_engine = engine
        net.zero_grad(set_to_none=True)
        loss = tr.step(sample, True)
        loss.backward()
        grads = torch.cat([p.grad.flatten().double() for p in net.parameters() if p.grad is not None])
        assert loss.dim() == 0 and tr.nb_iter == 1 and abs(float(tr.log_iter()["train_loss"]) - float(loss.detach())) < 1e-6
        assert "ref_img" in tr.ims and "scale_0_depth_est" in tr.ims
        out[engine] = (float(loss.detach()), grads)
    (lt, gt), (lp, gp) = out["torch"], out["pscv"]
    cos = float(torch.dot(gt, gp) / (gt.norm() * gp.norm()))
    print(architecture, supervised, "loss torch", lt, "pscv", lp, "cosine", cos)
    assert np.isfinite(lt) and abs(lp - lt) <= 1e-5 * abs(lt)
    assert gt.numel() == gp.numel() and cos >= 0.9999


def test_trainer_test_and_depthmap_eval_score_equal_torch(env):
    from wild_deep_mvs_amd import synthetic
    from wild_deep_mvs_amd.evaluation import depthmap_eval as E
    from wild_deep_mvs_amd.models.trainer import Trainer
    net = _net("mvsnet").eval()
    sample = _sample(synthetic)
    res = {}
    for engine in ("torch", "pscv"):
        tr = Trainer(net, _args())
        tr.loss_engine = engine
        tr.test(sample)
        assert set(tr.loss_means) == {"EPE", "1pxError", "3pxError"} and tr.nb_iter == 1
        res[engine] = {k: float(v) for k, v in tr.loss_means.items()}
    with torch.no_grad():
        out = net(*[sample[k].cuda() for k in ("imgs", "K", "R", "t", "depth_min", "depth_max")])
    acc = E.Scores()
    acc.add(E.score(out["depth"], sample["depth"][:, 0].cuda(), sample["mask"][:, 0].cuda(), sample["depth_min"].cuda(), sample["depth_max"].cuda()))
    acc.add(E.score(out["depth"], sample["depth"][:, 0].cuda(), sample["mask"][:, 0].cuda() > 0.5, sample["depth_min"].cuda(), sample["depth_max"].cuda()))
    res["score"] = acc.result()
    print(res)
    for k, want in res["torch"].items():
        assert abs(res["pscv"][k] - want) <= 1e-5 * abs(want) and abs(res["score"][k] - want) <= 1e-5 * abs(want), (k, res)
    assert res["torch"]["EPE"] > 0
