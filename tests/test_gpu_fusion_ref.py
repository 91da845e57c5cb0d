"""GPU: every pass of the depth-map fusion (pscv_fuse_depth_pass, csrc/depth_fusion.hip) against the float64 reference with derived
bounds of tests/_fusion_bounds.py, on the cases of tests/_fusion_cases.py that tests/test_gpu_fusion.py does not run: N = 2, a
one-row image, views narrower than a tile and of one pixel, bit 63 of the consistent-view mask, more than 1024 segments (the scan
kernel's per-thread loop), num_consistent 0 / N - 1 / N, non-finite depths and depths on the fp32 thresholds, used bytes other than
0 / 1, a non-zero top byte in the packed colour, rolled cameras, and the two dyadic cases that sit on a half-integer projection and on
the disparity threshold themselves.  Per pass: every decided emit flag, row-major order, positions within their own propagated
bound, colours exactly, every mark inside a candidate target and every decided mark present; no pixel is exempt.  Plus the whole run
against its passes and a side stream against the default one, bit for bit."""
import numpy as np
import pytest
import torch

from tests import _fusion_bounds as FB
from tests import _fusion_cases as FC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from wild_deep_mvs_amd import _lib as L, ops
    L.lib()
    return ops


def device_inputs(case):
    """(depths, colours, cams) on the GPU: uint8 [h,w,3] colours (packed by ops.pack_rgba8, top byte 0) unless the case sets a top byte"""
    dd = [torch.from_numpy(d).cuda() for d in case["depths"]]
    if case["alpha"] is None:
        cc = [torch.from_numpy(c).cuda() for c in case["colors"]]
    else:
        cc = [torch.from_numpy(p).cuda() for p in FC.packed_colors(case)]
    return dd, cc, torch.from_numpy(case["cams"]).cuda()


def kernel_step(ops, case):
    dd, cc, cg = device_inputs(case)

    def step(i, used):
        ug = [torch.from_numpy(u).cuda() for u in used]
        xyz, rgb, pix = ops.fuse_depth_pass(i, dd, cc, cg, ug, disp_thresh=case["disp_thresh"], num_consistent=case["num_consistent"])
        return xyz.cpu().numpy(), rgb.cpu().numpy(), pix.cpu().numpy(), [u.cpu().numpy() for u in ug]
    return step


def check_case(ops, name, on_pass=None):
    case = FC.get(name)
    bad, stats, und, tup = FB.run_case(case, kernel_step(ops, case), name=name, on_pass=on_pass)
    print(f"\n[fusion-ref] {name}: points {sum(s['points'] for s in stats)}, decided sets {sum(s['decided_sets'] for s in stats)} of "
          f"{sum(s['active'] for s in stats)} active, worst |kernel - ref| / bound {max(s['pos_ratio'] for s in stats):.4f}, "
          f"worst rel err {max(s['old_bar'] for s in stats):.3e}, worst rel bound {max(s['bound_rel'] for s in stats):.3e}, "
          f"undecided {sum(und.values())} of {tup}")
    assert not bad, "\n".join(bad[:20])
    assert sum(und.values()) <= FB.UNDECIDED_CAP * max(tup, 1)
    return stats


@pytest.mark.parametrize("name", FC.NEW)
def test_each_pass_matches_the_reference(ops, name):
    seen = {}

    def on_pass(i, ref, dec, got, before, after):
        FC.check_reached(name, i, ref, dec, got, before, after, seen)
    stats = check_case(ops, name, on_pass)
    FC.check_reached_end(name, stats, seen)


@pytest.mark.parametrize("name", ["segments_130x264", "n9_ragged_behind/p2"])
def test_whole_run_equals_its_passes(ops, name):
    """ops.fuse_depth_maps carries the device counter and the masks across passes: bit for bit the concatenation of per-pass launches"""
    case = FC.get(name)
    dd, cc, cg = device_inputs(case)
    kw = {"disp_thresh": case["disp_thresh"], "num_consistent": case["num_consistent"]}
    xyz, rgb, view, pix = ops.fuse_depth_maps(dd, cc, cg, want_pixel=True, **kw)
    used = [torch.zeros(d.shape, dtype=torch.uint8, device="cuda") for d in dd]
    parts = [ops.fuse_depth_pass(i, dd, cc, cg, used, **kw) for i in range(len(dd))]
    assert sum(p[0].shape[0] > 0 for p in parts) >= 2 and xyz.shape[0] > 1000
    assert torch.equal(xyz, torch.cat([p[0] for p in parts]))
    assert torch.equal(rgb, torch.cat([p[1] for p in parts]))
    assert torch.equal(pix, torch.cat([p[2] for p in parts]))
    want_view = torch.cat([torch.full((p[0].shape[0],), i, dtype=torch.int32, device="cuda") for i, p in enumerate(parts)])
    assert torch.equal(view, want_view)


def test_side_stream_equals_default_stream(ops):
    case = FC.get("n3/p1")
    dd, cc, cg = device_inputs(case)
    kw = {"disp_thresh": case["disp_thresh"], "num_consistent": case["num_consistent"], "want_pixel": True}
    a = ops.fuse_depth_maps(dd, cc, cg, **kw)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        b = ops.fuse_depth_maps(dd, cc, cg, **kw)
    side.synchronize()
    assert a[0].shape[0] > 1000
    for x, y in zip(a, b):
        assert x.shape == y.shape and torch.equal(x, y)
