"""pscv_cvp_depth_hypos (csrc/depth_hypo.hip: per-pixel fp64 steps, 8-pass multi-workgroup radix select, planes) held to the float64
reference of tests/_depth_hypo_ref.py (tests/test_depth_hypo_ref_cpu.py checks the reference and measures the bar without a GPU).

Per case, through ``ops.cvp_depth_hypos(..., want_steps=True)`` with fp64 constants built on the host:
  * the median step inside STEP_BAR (8 x the distance between two float64 evaluations; every rank error of the few-valid cases moves
    it by more than 10 %), the fallback exactly;
  * every plane within one fp32 ulp of float32(d + (k - 4) s), bit-equal away from rounding ties; NaN and inf where the depth has them.
The map is 72 x 97: two select workgroups, a ragged last block.  A batch item equals the same item run alone bit for bit."""
import numpy as np
import pytest
import torch

import _depth_hypo_ref as DR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from wild_deep_mvs_amd import _lib as L, ops
    L.lib()
    return L, ops


def run(ops, depth, cams, fallback):
    hyp, steps = ops.cvp_depth_hypos(torch.from_numpy(np.ascontiguousarray(depth)).cuda(), torch.from_numpy(np.ascontiguousarray(cams)).cuda(),
                                     torch.from_numpy(np.ascontiguousarray(fallback)).cuda(), want_steps=True)
    return hyp.cpu().numpy(), steps.cpu().numpy()


def check_case(ops, tag, depth, cams, fallback):
    hyp, steps = run(ops, depth, cams, fallback)
    r = DR.reference(depth, cams, fallback)
    with np.errstate(all="ignore"):
        rel = [abs(g - s) / abs(s) if n else 0.0 for g, s, n in zip(steps, r["steps"], r["n_valid"])]
    print(f"[parity] depth hypo {tag}: n_valid {r['n_valid'].tolist()}, steps {steps.tolist()}, relative distance {['%.2e' % v for v in rel]}, "
          f"worst {max(rel) / DR.STEP_BAR:.3f} of the bar {DR.STEP_BAR:.2e}", flush=True)
    DR.check_steps(tag, steps, r)
    ties, diff = DR.check_planes(tag, hyp, r)
    print(f"[parity] depth hypo {tag}: {hyp.size} planes, {ties} within 1e-9 of a rounding tie, {diff} differ (by one ulp)", flush=True)
    return hyp, steps, r


@pytest.mark.parametrize("name", [c for c in DR.CASES if c != "batch"])
def test_depth_hypos_against_float64(env, name):
    L, ops = env
    depth, cams, fallback = DR.inputs(name)
    hyp, steps, r = check_case(ops, name, depth, cams, fallback)
    if name.startswith("valid-") and name[6:].isdigit() and int(name[6:]) > 0:
        n = int(name[6:])
        assert int(np.argmin(np.abs(r["sorted"][0] - steps[0]))) == DR.EXPECT_RANK[n]      # the lower median, not a neighbouring rank


def test_depth_hypos_batch_items_equal_the_items_alone(env):
    """B = 3: an all-invalid item (fallback), one with 2 valid pixels, a full one -- each equals itself run alone bit for bit."""
    L, ops = env
    depth, cams, fallback = DR.inputs("batch")
    hyp, steps, r = check_case(ops, "batch", depth, cams, fallback)
    assert r["n_valid"].tolist() == [0, 2, DR.H * DR.W]
    for b in range(3):
        h1, s1 = run(ops, depth[b:b + 1], cams[b:b + 1], fallback[b:b + 1])
        assert s1[0] == steps[b], (b, s1[0], steps[b])
        assert np.array_equal(h1[0].view(np.uint32), hyp[b].view(np.uint32)), f"item {b} differs from itself run alone"
