"""The float64 reference of tests/_depth_hypo_ref.py, checked WITHOUT a GPU against oracle.cvpmvsnet.cal_depth_hypo (pinned to the
reference project by tests/test_oracle_cvp.py), per batch item:
  * the planes agree to the oracle's own fp32 accumulation, the valid count and the fallback exactly;
  * the worst relative distance between the two float64 steps is THE measurement behind the GPU bar: it stays inside STEP_DIST, and
    STEP_BAR = 8 STEP_DIST stays below 1e-9;
  * the few-valid cases pick the lower median (lower of two, second of four, third of five) and every neighbouring rank would move the
    step by more than 10 %; the two-level tie case returns the majority level's step."""
import numpy as np
import pytest
import torch

import _depth_hypo_ref as DR
from oracle import cvpmvsnet as OC

WORST = {}


def oracle_item(c, b):
    s = slice(b, b + 1)
    hyp, iv = OC.cal_depth_hypo(c["depth"][s], c["ref_in"][s], c["src_in"][s], c["ref_ex"][s], c["src_ex"][s], c["dmin"][s], c["dmax"][s],
                                want_interval=True)
    return hyp[0].numpy(), float(iv[0])


@pytest.mark.parametrize("name", DR.CASES)
def test_reference_against_the_oracle(name):
    c = DR.make_case(name)
    depth, cams, fallback = DR.inputs(c)
    r = DR.reference(depth, cams, fallback)
    for b in range(depth.shape[0]):
        hyp, iv = oracle_item(c, b)
        n, s = int(r["n_valid"][b]), float(r["steps"][b])
        if n == 0:
            assert s == iv == float(fallback[b]), (name, b, s, iv)
            rel = 0.0
        else:
            rel = abs(s - iv) / abs(iv)
        WORST[(name, b)] = rel
        print(f"[parity] depth hypo ref {name}[{b}]: n_valid {n}, step {s!r}, oracle {iv!r}, relative distance {rel:.3e} "
              f"({rel / DR.STEP_DIST:.3f} of STEP_DIST)", flush=True)
        assert rel <= DR.STEP_DIST, (name, b, rel)
        fin = np.isfinite(r["planes64"][b])
        assert np.array_equal(np.isnan(hyp), np.isnan(r["planes64"][b])) and np.array_equal(hyp[~fin & ~np.isnan(hyp)], r["planes"][b][~fin & ~np.isnan(hyp)])
        # the oracle adds k * interval to an fp32 map in fp32: two roundings of values up to |d| + 4 s
        tol = 2.0 ** -23 * (np.abs(depth[b].astype(np.float64)) + 4.0 * s)[None].repeat(8, 0)
        with np.errstate(invalid="ignore"):
            assert np.all(np.abs(hyp.astype(np.float64) - r["planes64"][b])[fin] <= tol[fin]), name


def test_the_bar_is_below_the_tie_rule():
    assert DR.STEP_BAR == 8.0 * DR.STEP_DIST and DR.STEP_BAR < 1e-9


@pytest.mark.parametrize("n", DR.FEW)
def test_few_valid_pixels_pick_the_lower_median(n):
    depth, cams, fallback = DR.inputs(f"valid-{n}")
    r = DR.reference(depth, cams, fallback)
    assert int(r["n_valid"][0]) == n
    assert np.array_equal(np.flatnonzero(r["valid"][0].reshape(-1)), np.sort(np.asarray(DR.FEW_PIX[:n], dtype=np.int64)))
    if n == 0:
        assert r["steps"][0] == float(fallback[0])
        return
    vals = r["sorted"][0]
    assert r["steps"][0] == vals[DR.EXPECT_RANK[n]]
    assert np.all(vals[1:] / vals[:-1] > 1.1), vals          # a wrong rank moves the step by more than 10 %


def test_full_maps_and_ties():
    for name, want in (("valid-all-but-one", DR.H * DR.W - 1), ("valid-all", DR.H * DR.W), ("tie-constant", DR.H * DR.W),
                       ("tie-two-levels", DR.H * DR.W), ("non-finite", DR.H * DR.W - 10)):
        depth, cams, fallback = DR.inputs(name)
        r = DR.reference(depth, cams, fallback)
        assert int(r["n_valid"][0]) == want, (name, int(r["n_valid"][0]))
        if name == "tie-constant":           # every key shares its leading bytes: the select's last passes decide
            bits = r["sorted"][0].view(np.uint64)
            assert int(bits.max() ^ bits.min()) < (1 << 16) and bits.max() != bits.min(), hex(int(bits.max() ^ bits.min()))
        if name == "tie-two-levels":         # 40 % at depth 3, 60 % at depth 5: the median is a step of the majority level
            lvl5 = r["abs_step"][0][depth[0] == 5.0]
            assert lvl5.min() <= r["steps"][0] <= lvl5.max() and not np.any(np.isclose(r["abs_step"][0][depth[0] == 3.0], r["steps"][0], rtol=1e-3))
        if name == "non-finite":
            bad = ~np.isfinite(depth[0])
            assert not r["valid"][0][bad].any() and int(np.isnan(r["planes"][0][:, bad]).sum()) == 8 * 5 and int(np.isinf(r["planes"][0][:, bad]).sum()) == 8 * 5
    depth, cams, fallback = DR.inputs("batch")
    assert [int(n) for n in DR.reference(depth, cams, fallback)["n_valid"]] == [0, 2, DR.H * DR.W]
