"""tests/_softargmin_ref.py pinned to the committed oracles and goldens, its merge and window rules checked against its own
full-range results, and every case of tests/test_gpu_softargmin_ref.py checked from float64 alone: the share of pixels whose
confidence is allowed a second value stays below the cap.  No GPU."""
import numpy as np
import pytest
import torch

import _softargmin_ref as R
import test_gpu_softargmin_ref as G
from _util import load_golden, t


def _rand(B=2, D=16, h=9, w=13, sigma=3.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, D, h, w, generator=g) * sigma, g


def test_reference_matches_the_mvsnet_oracle():
    """oracle.mvsnet.regress / photometric_confidence (fp32 torch) against the float64 reference; pixels whose index lies within
    1e-4 of an integer may take the neighbouring window (the oracle truncates an fp32 index)."""
    from oracle import mvsnet as O
    lg, g = _rand(seed=1)
    dv = torch.rand(2, 16, generator=g) * 3 + 1
    prob, depth, conf = O.regress(lg, dv)
    ref = R.Ref(lg, dv)
    np.testing.assert_allclose(prob.numpy(), ref.prob, atol=2e-7)
    np.testing.assert_allclose(depth.numpy(), ref.depth, atol=4e-6)
    mask, alts = ref.fragile(0, 1e-4)
    err = np.minimum(np.abs(conf.numpy() - ref.conf0()), np.where(mask, np.abs(conf.numpy() - alts[0]), np.inf))
    assert err.max() <= 1e-6 and mask.mean() < 0.01
    np.testing.assert_allclose(O.photometric_confidence(prob).numpy(), conf.numpy(), atol=0)


@pytest.mark.parametrize("window", [2.0, 2.5])
def test_reference_matches_the_vis_oracle(window):
    from oracle import vismvsnet as OV
    lg, _ = _rand(seed=2)
    prob, idx, conf = OV.soft_argmin(lg.double(), window)
    ref = R.Ref(lg)
    np.testing.assert_allclose(prob.numpy(), ref.prob, atol=1e-15)
    np.testing.assert_allclose(idx[:, 0].numpy(), ref.index, atol=1e-13)
    np.testing.assert_allclose(conf[:, 0].numpy(), ref.conf1(window), atol=1e-14)
    np.testing.assert_allclose(OV.entropy(prob)[:, 0].numpy(), ref.entropy(), atol=1e-14)
    # the clamp matters only where p < 1e-9
    peaked = R.Ref(lg * 20)
    assert (peaked.prob < 1e-9).any() and np.abs(peaked.entropy() - peaked.entropy(clamp=False)).max() > 0
    np.testing.assert_allclose(OV.entropy(torch.softmax((lg * 20).double(), 1))[:, 0].numpy(), peaked.entropy(), atol=1e-14)


@pytest.mark.parametrize("fname", ["mvsnet_tiny.npz", "mvsnet_s_tiny.npz"])
def test_reference_matches_the_goldens(fname):
    g = load_golden(fname)
    lg = t(g["logits"]).squeeze(1)
    dv = t(g["depth_values"])[:, 0]
    ref = R.Ref(lg, dv)
    np.testing.assert_allclose(g["depth"], ref.depth, atol=2e-6 * float(dv.max()))
    mask, alts = ref.fragile(0, 1e-4)
    got = g["photometric_confidence"]
    err = np.minimum(np.abs(got - ref.conf0()), np.where(mask, np.abs(got - alts[0]), np.inf))
    assert err.max() <= 1e-6


def test_softmax_semantics_of_infinities_and_nan():
    lg, _ = _rand(B=1, D=9, h=2, w=3, seed=3)
    lg[0, 2, 0, 0] = float("-inf")
    lg[0, :, 0, 1] = float("-inf")
    lg[0, 4, 1, 0] = float("inf")
    lg[0, 5, 1, 1] = float("nan")
    ref = R.Ref(lg, torch.arange(9.0).view(1, 9) + 1)
    want = torch.softmax(lg.double(), 1).numpy()
    assert np.array_equal(np.isnan(want), np.isnan(ref.prob))
    np.testing.assert_allclose(np.nan_to_num(want), np.nan_to_num(ref.prob), atol=1e-15)
    assert ref.prob[0, 2, 0, 0] == 0.0
    bad = np.zeros((1, 2, 3), bool)
    bad[0, 0, 1] = bad[0, 1, 0] = bad[0, 1, 1] = True
    for out in (ref.depth, ref.index, ref.entropy(), ref.conf0(), ref.conf1(2.0)):
        assert np.array_equal(np.isnan(out), bad)
    p = ref.partials()
    assert np.isneginf(p[0, 0, 0, 1]) and (p[0, 1:, 0, 1] == 0).all()


@pytest.mark.parametrize("D,sizes", [(192, (100, 57, 35)), (257, (100, 57, 100)), (41, (1, 39, 1))])
@pytest.mark.parametrize("per_pixel", [False, True])
def test_merge_of_uneven_shards_is_the_full_range(D, sizes, per_pixel):
    lg, g = _rand(B=2, D=D, h=5, w=7, sigma=4.0, seed=D)
    lg[:, sizes[0]:sizes[0] + sizes[1], 0, :] = float("-inf")           # one row: the middle shard is all -inf
    planes = torch.rand(2, D, 5, 7, generator=g) + 2 if per_pixel else torch.rand(2, D, generator=g) + 2
    full = R.Ref(lg, planes)
    b = np.concatenate([[0], np.cumsum(sizes)])
    parts = [R.Ref(lg[:, a:e], planes[:, a:e], int(a)).partials() for a, e in zip(b[:-1], b[1:])]
    assert np.isneginf(parts[1][:, 0, 0]).all()
    m = R.merge(parts)
    np.testing.assert_allclose(m["depth"], full.depth, atol=1e-12, rtol=0)
    np.testing.assert_allclose(m["index"], full.index, atol=1e-12, rtol=0)
    np.testing.assert_array_equal(m["max"], full.m)
    np.testing.assert_allclose(m["z"], full.z, rtol=1e-13)
    for window in (2.0, 2.5):
        tot = sum(R.window_shard(lg[:, a:e], m["max"], m["z"], full.index, window, int(a)) for a, e in zip(b[:-1], b[1:]))
        np.testing.assert_allclose(tot, full.conf1(window), atol=1e-13, rtol=0)


def test_fragile_names_the_value_on_the_other_side():
    """Constant logits, odd D: the index is exactly (D-1)/2; mode 0 may truncate one lower, window 2.0 may lose either edge plane."""
    D = 41
    ref = R.Ref(torch.full((1, D, 1, 2), 1.25))
    assert abs(ref.lidx[0, 0, 0] - 20.0) < 1e-12
    mask, alts = ref.fragile(0, 1e-6)
    assert mask.all() and abs(ref.conf0()[0, 0, 0] - 4 / D) < 1e-15 and abs(alts[0][0, 0, 0] - 4 / D) < 1e-15
    edge = R.Ref(torch.tensor([0.0, 0.0, -80.0, -80.0]).view(1, 4, 1, 1))            # index 0.5: trunc 0 -> planes 0..2; never 1
    assert not edge.fragile(0, 1e-6)[0].any()
    mask, alts = ref.fragile(1, 1e-6, 2.0)
    assert mask.all() and round(float(ref.conf1(2.0)[0, 0, 0]) * D) in (4, 5)        # (the float64 index itself is 20 +- 4e-15)
    assert sorted(round(float(a[0, 0, 0]) * D) for a in alts) == [4, 4, 5]
    mask, _ = ref.fragile(1, 1e-6, 2.5)
    assert not mask.any()
    # away from every edge the alternatives are the reference itself
    lg, _ = _rand(seed=5)
    r2 = R.Ref(lg)
    for mode, window in G.CONF:
        mask, alts = r2.fragile(mode, 1e-7, window)
        for a in alts:
            assert np.array_equal(a[~mask], r2.conf(mode, window)[~mask])


@pytest.mark.parametrize("case", G.CASES, ids=G.case_id)
def test_fragile_share_of_every_gpu_case(case):
    """The cap of the GPU file, from the reference alone, for every grid, offset and confidence mode a case runs with.  The
    constructed boundary cases (peaked, extreme, constant logits: the index sits ON an integer) are exempt: there it is the point."""
    for grid in G.GRIDS:
        lg = G.make_logits(case, grid)
        assert torch.equal(lg.to(G.DTYPES[case.dtype]).float(), lg)
        for offset in case.offsets:
            ref = R.Ref(lg, None, offset)
            assert not ref.bad.any()
            for mode, window in G.CONF:
                mask, _ = ref.fragile(mode, G.index_eps(case.D, offset), window)
                share = float(mask.mean())
                if case.regime == "near_integer" and mode == 0:
                    frac = ref.lidx - np.floor(ref.lidx)
                    assert np.all(np.minimum(frac, 1 - frac) > 0.5 * G.NEAR) and np.all(np.minimum(frac, 1 - frac) < 2 * G.NEAR)
                    assert share == 0.0, f"{G.case_id(case)}: an index {G.NEAR} from an integer must not be fragile (eps {G.index_eps(case.D, offset):.2e})"
                if case.regime == "constant":
                    assert np.all(np.abs(ref.lidx - (case.D - 1) / 2) < 1e-12)
                    assert bool(mask.all()) == (mode == 0 or window == 2.0)
                if case.capped:
                    assert share <= G.FRAGILE_CAP, f"{G.case_id(case)} grid {grid} offset {offset} mode {mode} window {window}: fragile share {share:.3f}"


def test_case_table_covers_what_it_claims():
    ds = {c.D for c in G.CASES if c.family == "slice"}
    assert ds == {1, 9, 41, 33, 40, 64, 192, 256, 257, 300}
    assert {c.dtype for c in G.CASES if c.family == "slice" and c.D == 257} == {"fp32", "fp16", "bf16"}
    assert {c.D for c in G.CASES if c.family == "small"} == {1, 8, 9, 16, 17, 32, 33}
    assert {c.regime for c in G.CASES if c.family == "regime"} == {"flat", "peaked", "extreme", "constant", "near_integer"}
    for D in (257, 300):
        assert (D + 7) // 8 > 32                                     # slices longer than SA_PMAX: the two-pass loop
    assert (256 + 7) // 8 == 32
