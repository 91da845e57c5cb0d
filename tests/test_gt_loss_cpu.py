"""CPU: the loss reductions and depth-map scores.  The numpy restatement tests/_gt_loss_ref.py must equal
the fixture tests/golden/gtloss_tiny.npz (expectations from the reference's own functions and torch's ``F.interpolate``) and torch
autograd of the reference's formulas; every new export must reject bad arguments on the host, before any launch, with a message."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _gt_loss_ref as R
from wild_deep_mvs_amd import _lib as L
from wild_deep_mvs_amd import ops

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gtloss_tiny.npz")
SIZES = {"s1": (24, 48), "s2": (12, 24), "s4": (6, 12), "s3": (8, 16), "s21": (12, 48)}


@pytest.fixture(scope="module")
def z():
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


def test_restatement_terms_equal_the_fixture(z):
    terms = R.fixture_terms(z)
    assert len(terms) == 20 and {t["kind"] for t in terms} == {R.GT_PLAIN, R.GT_BAYES, R.L_PLAIN, R.L_BAYES}
    for i, t in enumerate(terms):
        got = R.term_of(t, np.float64)
        assert abs(got["value"] - t["want"]) <= 1e-12 * max(1.0, abs(t["want"])), (i, got["value"], t["want"])
        # the fp32-per-pixel form the kernel is compared with stays within fp32 rounding of it
        assert abs(R.term_of(t)["value"] - t["want"]) <= 2e-6 * max(1.0, abs(t["want"])), i
    for s in SIZES:
        assert R.term_of(next(t for t in terms if t["a"] is z[f"{s}_d"]))["sums"][2] == float(z[f"{s}_count"])
    empty = terms[-1]
    assert R.term_of(empty)["sums"][2] == 0 and R.term_of(empty)["norm"] == 1.0 and R.term_of(empty)["value"] == 0.0


def test_restatement_down_masks_and_ground_truth_equal_torch(z):
    for s, (h, w) in SIZES.items():
        g, m = R.gt_down(z["gt"], z["gt_mask"], h, w)
        assert m.dtype == np.bool_ and np.array_equal(m, z[f"{s}_mask_down"]), s
        want = z[f"{s}_gt_down"]
        assert g.dtype == np.float32 and np.all(np.abs(g - want) <= 2e-7 * np.abs(want)), s
        inv = R.invalid_taps(z["gt_mask"], h, w)
        ntaps = (1 if (24 // h) % 2 else 2) * (1 if (48 // w) % 2 else 2)
        assert all((inv == k).any() for k in range(0, min(ntaps, 3) + 1)), s
    with pytest.raises(ValueError, match="non-integer"):
        R.gt_down(z["gt"], z["gt_mask"], 7, 13)
    assert 2 * 24 * 48 > 1024 and (2 * 24 * 48) % 1024        # more than one block of the reduce launch, the last one ragged


def test_restatement_tap_rule_equals_interpolate_for_other_ratios():
    rng = np.random.default_rng(0)
    for rh, rw in [(1, 1), (2, 2), (3, 3), (4, 4), (5, 5), (8, 8), (2, 1), (6, 3), (12, 2), (3, 4)]:
        h, w = 3, 5
        gt = rng.uniform(1, 5, (2, h * rh, w * rw)).astype(np.float32)
        mask = (rng.random(gt.shape) > 0.2).astype(np.float32)
        g, m = R.gt_down(gt, mask, h, w)
        tg = F.interpolate(torch.from_numpy(gt)[:, None], size=(h, w), mode="bilinear", align_corners=False)[:, 0].numpy()
        tm = (F.interpolate(torch.from_numpy(mask)[:, None], size=(h, w), mode="bilinear", align_corners=False) == 1)[:, 0].numpy()
        assert np.array_equal(m, tm) and np.all(np.abs(g - tg) <= 2e-7 * np.abs(tg)), (rh, rw)


def test_restatement_gradients_equal_autograd_of_the_reference_formulas(z):
    from wild_deep_mvs_amd.models.utils import bayesian_version_loss
    g_up = 0.7
    for i, t in enumerate(R.fixture_terms(z)):
        a = torch.tensor(t["a"], dtype=torch.float64, requires_grad=True)
        u = None if t["u"] is None else torch.tensor(t["u"], dtype=torch.float64, requires_grad=True)
        if t["kind"] in (R.GT_PLAIN, R.GT_BAYES):
            b, (h, w) = a.shape[0], a.shape[-2:]
            gt = F.interpolate(torch.tensor(t["gt"], dtype=torch.float64)[:, None], size=(h, w), mode="bilinear", align_corners=False)
            m = (F.interpolate(torch.tensor(t["mask"], dtype=torch.float64)[:, None], size=(h, w), mode="bilinear", align_corners=False) == 1).double()
            l = torch.abs(a.reshape(b, 1, h, w) - gt) / torch.tensor(t["interval"], dtype=torch.float64).view(b, 1, 1, 1)
            uu = None if u is None else u.reshape(b, 1, h, w)
        else:
            l, m, uu = a, torch.tensor(np.asarray(t["mask"], dtype=np.float64)), u
        if t["kind"] in (R.GT_BAYES, R.L_BAYES):
            value = bayesian_version_loss(l, uu, m)
        else:
            total, count = torch.sum(l * m), torch.sum(m)
            value = total / count if (t["kind"] == R.GT_PLAIN or count != 0) else total
        (g_up * t["factor"] * value).backward()
        da, du = R.grads_of(t, g_up, np.float64)
        assert np.allclose(da, a.grad.numpy(), rtol=1e-10, atol=1e-14), i
        if u is not None:
            assert np.allclose(du, u.grad.numpy(), rtol=1e-10, atol=1e-14), i
        else:
            assert du is None
        valid = R.pixel_loss(t["kind"], t["a"], t["gt"], t["mask"], t["interval"])[1].reshape(da.shape)
        assert np.all(da[~valid] == 0)
    # d == gt_down: sign(0) = 0
    s1 = R.fixture_terms(z)[0]
    assert np.all(R.grads_of(s1)[0][:, 1, 2] == 0) and np.abs(R.grads_of(s1)[0]).max() > 0


def test_restatement_scores_equal_the_fixture(z):
    step = (z["m_max"][:, 0] - z["m_min"][:, 0]) / np.float32(128)
    thr, rel = tuple(z["m_thresholds"]), tuple(z["m_rel_thresholds"])
    for name in ("m4", "m1", "mf"):
        est = z[f"{name}_est"]
        assert R.threshold_margin(est, z["m_gt"], z["m_mask"], step, thr, rel) > 1e-3, name
        got = R.metrics(est, z["m_gt"], z["m_mask"], step, thr, rel)
        assert np.array_equal(got["sums"][:, 0], z[f"{name}_count"])
        assert np.array_equal(got["sums"][:, 2:4], z[f"{name}_thres_counts"]) and np.array_equal(got["sums"][:, 8:10], z[f"{name}_rel_counts"])
        for key in ("EPE", "Rel", "SqRel"):
            assert abs(got[key] - z[f"{name}_{key}"]) <= 1e-5 * abs(z[f"{name}_{key}"]), (name, key)
        assert np.allclose(got["thres"], z[f"{name}_thres"], rtol=0, atol=1e-6) and np.allclose(got["rel_thres"], z[f"{name}_rel_thres"], rtol=0, atol=1e-6)
    assert np.array_equal(R.upsample(z["m1_est"], 24, 48), z["m1_est"])          # h = H: a copy
    empty = R.metrics(z["m4_est"], z["m_gt"], np.zeros_like(z["m_mask"]), step)
    assert np.isnan(empty["EPE"]) and np.isnan(empty["thres"]).all()


# ---- the exports' argument checks: no GPU needed, nothing is launched --------------------------------------------------------------
class _Table:
    """Parallel host arrays of n terms that point at host scratch (never read: every case below is rejected before a launch)."""

    def __init__(self, n, kind=1, dims=(2, 6, 12, 24, 48)):
        self.scratch = (C.c_double * 8)()
        p = C.addressof(self.scratch)
        self.n = n
        self.kinds, self.u8 = (C.c_int * n)(*[kind] * n), (C.c_int * n)(*[0] * n)
        self.dims, self.factors = (C.c_long * (5 * n))(*list(dims) * n), (C.c_float * n)(*[1.0] * n)
        self.a, self.u, self.gt, self.mask, self.interval, self.ga, self.gu = ((C.c_void_p * n)(*[p] * n) for _ in range(7))
        self.p = p

    def fwd(self, **kw):
        args = dict(n=self.n, kinds=self.kinds, a=self.a, u=self.u, gt=self.gt, mask=self.mask, interval=self.interval, u8=self.u8,
                    dims=self.dims, factors=self.factors, ws=self.p, loss=self.p, term=self.p, sums=self.p, norm=self.p)
        args.update(kw)
        return L.lib().pscv_loss_terms(*[args[k] for k in ("n", "kinds", "a", "u", "gt", "mask", "interval", "u8", "dims", "factors", "ws",
                                                            "loss", "term", "sums", "norm")], None)

    def bwd(self, **kw):
        args = dict(n=self.n, kinds=self.kinds, a=self.a, u=self.u, gt=self.gt, mask=self.mask, interval=self.interval, u8=self.u8,
                    dims=self.dims, factors=self.factors, norm=self.p, g=self.p, ga=self.ga, gu=self.gu)
        args.update(kw)
        return L.lib().pscv_loss_terms_bwd(*[args[k] for k in ("n", "kinds", "a", "u", "gt", "mask", "interval", "u8", "dims", "factors",
                                                                "norm", "g", "ga", "gu")], None)


def _err():
    return L.lib().pscv_last_error().decode()


@pytest.mark.parametrize("which", ["fwd", "bwd"])
def test_loss_exports_reject_bad_arguments(which):
    name = "pscv_loss_terms" + ("_bwd" if which == "bwd" else "")
    call = lambda tab, **kw: getattr(tab, which)(**kw)
    for key in ("kinds", "a", "u", "gt", "mask", "interval", "u8", "dims", "factors"):                    # a null table array
        assert call(_Table(2), **{key: None}) != 0 and name in _err() and "null pointer" in _err(), key
    for key in (("ws", "loss", "term", "sums", "norm") if which == "fwd" else ("norm", "g")):             # a null output / input
        assert call(_Table(2), **{key: None}) != 0 and "null pointer" in _err(), key
    if which == "bwd":
        assert call(_Table(2), ga=None, gu=None) != 0 and "null pointer" in _err()
    for key in ("a", "u", "gt", "mask", "interval"):                                                        # a null entry of term 1
        tab = _Table(2)
        getattr(tab, key)[1] = None
        assert call(tab) != 0 and "term 1" in _err() and "null pointer" in _err(), key
    tab = _Table(2, kind=L.LOSS_L_PLAIN)                   # ... but what a kind does not use may be null
    for key in ("u", "gt", "interval"):
        getattr(tab, key)[0] = None
    tab.a[1] = None
    assert call(tab) != 0 and "term 1" in _err()
    assert call(_Table(33)) != 0 and "33 terms" in _err() and "32" in _err()
    assert call(_Table(1), n=0) != 0 and "no terms" in _err()
    assert call(_Table(2, dims=(2, 7, 13, 24, 48))) != 0 and "non-integer ratio" in _err()
    assert call(_Table(2, dims=(2, 6, 12, 24, 50))) != 0 and "non-integer ratio" in _err()
    for dims in [(0, 6, 12, 24, 48), (2, 0, 12, 24, 48), (2, 6, 0, 24, 48), (2, 6, 12, 0, 48), (2, 6, 12, 24, 0), (2, -6, 12, 24, 48)]:
        assert call(_Table(2, dims=dims)) != 0 and "size" in _err(), dims
    assert call(_Table(1, dims=(1 << 12, 1 << 10, 1 << 10, 1 << 10, 1 << 10))) != 0 and "2^31" in _err()
    assert call(_Table(2, kind=7)) != 0 and "unknown kind" in _err()


def test_workspace_exports_reject_bad_arguments():
    lib = L.lib()
    dims = (C.c_long * 10)(2, 24, 48, 24, 48, 2, 6, 12, 24, 48)
    assert lib.pscv_loss_terms_workspace(2, dims) == (3 + 1) * 3 * 8              # 2304 and 144 pixels: three blocks and one
    assert lib.pscv_loss_terms_workspace(2, None) < 0 and "null pointer" in _err()
    assert lib.pscv_loss_terms_workspace(33, dims) < 0 and "33 terms" in _err()
    assert lib.pscv_loss_terms_workspace(0, dims) < 0
    assert lib.pscv_loss_terms_workspace(1, (C.c_long * 5)(2, 0, 48, 24, 48)) < 0 and "size" in _err()
    assert lib.pscv_depth_metrics_workspace(2, 24, 48) == 2 * 2 * L.METRIC_SUMS * 8
    for b, H, W in [(0, 24, 48), (2, 0, 48), (2, 24, 0), (2, -1, 48)]:
        assert lib.pscv_depth_metrics_workspace(b, H, W) < 0 and "size" in _err()


def test_depth_metrics_export_rejects_bad_arguments():
    lib = L.lib()
    scratch = (C.c_double * 8)()
    p = C.addressof(scratch)
    thr = (C.c_float * 4)(1, 3, 0, 0)
    good = dict(est=p, gt=p, mask=p, u8=0, step=p, b=2, h=6, w=12, H=24, W=48, ta=thr, na=2, tr=thr, nr=1, ws=p, sums=p, means=p)
    order = ("est", "gt", "mask", "u8", "step", "b", "h", "w", "H", "W", "ta", "na", "tr", "nr", "ws", "sums", "means")
    call = lambda **kw: lib.pscv_depth_metrics(*[dict(good, **kw)[k] for k in order], None)
    for key in ("est", "gt", "mask", "ws", "sums", "means"):
        assert call(**{key: None}) != 0 and "pscv_depth_metrics" in _err() and "null pointer" in _err(), key
    assert call(ta=None) != 0 and "null pointer" in _err() and call(tr=None) != 0 and "null pointer" in _err()
    for key in ("b", "h", "w", "H", "W"):
        assert call(**{key: 0}) != 0 and "size" in _err(), key
    assert call(na=5) != 0 and "thresholds" in _err() and call(nr=5) != 0 and "thresholds" in _err() and call(na=-1) != 0


def test_ops_raise_on_cpu_tensors_and_on_too_many_terms_or_thresholds(z):
    d, gt, m = torch.zeros(2, 6, 12), torch.ones(2, 24, 48), torch.ones(2, 24, 48)
    term = ops.LossTerm(L.LOSS_GT_PLAIN, 1.0, d, m, gt=gt, interval=torch.ones(2))
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.loss_terms([term])
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.loss_terms([ops.LossTerm(L.LOSS_L_BAYES, 1.0, d, d > 0, u=d)])
    with pytest.raises(L.PscvError, match="33 terms"):
        ops.loss_terms([term] * 33)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.depth_metrics(d, gt, m, torch.ones(2))
    with pytest.raises(L.PscvError, match="thresholds"):
        ops.depth_metrics(d, gt, m, thresholds=(1, 2, 3, 4, 5))
    with pytest.raises(TypeError):
        ops.depth_metrics(d, gt, m.double())
    assert (L.LOSS_GT_PLAIN, L.LOSS_GT_BAYES, L.LOSS_L_PLAIN, L.LOSS_L_BAYES) == (R.GT_PLAIN, R.GT_BAYES, R.L_PLAIN, R.L_BAYES)
    assert L.LOSS_MAX_TERMS == R.MAX_TERMS == 32 and L.METRIC_MAX_THRESH == R.MAX_THRESH == 4 and L.METRIC_SUMS == 12


def test_trainer_loss_engine_defaults_to_torch():
    from wild_deep_mvs_amd.models.trainer import Trainer
    from wild_deep_mvs_amd.evaluation import depthmap_eval as E
    from wild_deep_mvs_amd import training as T
    assert Trainer.loss_engine == "torch" and Trainer().loss_engine == "torch"
    assert issubclass(T.LossTermsFn, torch.autograd.Function) and callable(E.score) and E.NAMES == ("EPE", "1pxError", "3pxError")
    with pytest.raises(RuntimeError, match="no CPU"):
        E.score(torch.zeros(1, 6, 12), torch.ones(1, 24, 48), torch.ones(1, 24, 48), torch.ones(1, 3), torch.full((1, 3), 2.0))
