"""The forward half of tests/_warp_bwd_ref.py (``forward``, ``positions`` with ``ref_y0``, ``variance_partial``, ``fragile``) pinned
to the oracles' fp32 VALUES on the rigs of tests/test_warp_bwd_ref_cpu.py, at that file's bar, and every rig of
tests/test_gpu_warp_fwd.py checked from float64 alone: the fragile share below the cap, the staging mode a case names.  No GPU."""
import pytest
import torch

import _warp_bwd_ref as R
import _warp_fwd_rigs as G
from test_warp_bwd_ref_cpu import _assert_partly_behind, _cl, _compare, _homog_blocks, _proj, _rig


def _mvsnet_case(B=2, V=3, C=32, h=16, w=24, hs=14, ws=26, D=8, seed=5, sigma=0.5):
    from wild_deep_mvs_amd import ops
    K, Rm, t, dmin, dmax = _rig(B, V, h, w, hs, ws)
    proj = _proj(K, Rm, t)
    dv = dmin.view(B, 1) + (dmax - dmin).view(B, 1) * torch.arange(D).view(1, D) / (D - 1)
    cams = ops.proj_cams([proj[:, i] for i in range(1, V)], proj[:, 0])
    gen = torch.Generator().manual_seed(seed)
    ref = torch.randn(B, C, h, w, generator=gen) * sigma
    srcs = [torch.randn(B, C, hs, ws, generator=gen) * sigma for _ in range(V - 1)]
    return proj, dv, cams, ref, srcs


@pytest.mark.parametrize("cost", ["variance", "softmin", "warp_only"])
def test_forward_matches_mvsnet_oracle(cost):
    """PROJ geometry, per-batch planes, one camera turned by ~75 degrees: O.homo_warping + variance_cost / softmin_cost / the warp."""
    from oracle import mvsnet as O
    proj, dv, cams, ref, srcs = _mvsnet_case(sigma=0.3 if cost == "softmin" else 0.5)
    h, w = ref.shape[-2:]
    warped = [O.homo_warping(s, proj[:, i + 1], proj[:, 0], dv, (h, w)) for i, s in enumerate(srcs)]
    if cost == "variance":
        want = O.variance_cost(ref, warped).movedim(1, -1)
    elif cost == "softmin":
        want = O.softmin_cost(ref, warped, torch.tensor([0.7])).movedim(1, -1)
    else:
        want = torch.stack(warped).movedim(2, -1)
    got, ix, iy, qz = R.forward(None if cost == "warp_only" else _cl(ref), [_cl(s) for s in srcs], cams, dv, geom="proj", cost=cost, temp=0.7,
                                ref_hw=(h, w))
    _assert_partly_behind(ix, iy, qz, *srcs[0].shape[-2:])
    assert tuple(got.shape) == tuple(want.shape)
    _compare(f"forward {cost}", got, want)


def test_forward_matches_cvp_oracle_per_pixel_hypotheses():
    """PROJ geometry with per-pixel hypotheses, 16 channels: OC.homo_warping + OC.variance_cost (the CVP rounding order)."""
    from oracle import cvpmvsnet as OC
    from wild_deep_mvs_amd import ops
    B, V, C, h, w, D = 2, 3, 16, 12, 18, 6
    K, Rm, t, dmin, dmax = _rig(B, V, h, w, h, w)
    E = torch.zeros(B, V, 4, 4)
    E[..., :3, :3], E[..., :3, 3:], E[..., 3, 3] = Rm, t, 1.0
    proj = _proj(K, Rm, t)
    cams = ops.proj_cams([proj[:, i] for i in range(1, V)], proj[:, 0])
    gen = torch.Generator().manual_seed(6)
    planes = dmin.view(B, 1) + (dmax - dmin).view(B, 1) * torch.arange(D).view(1, D) / (D - 1)
    hyp = (planes.view(B, D, 1, 1) * (1.0 + 0.2 * (torch.rand(B, D, h, w, generator=gen) - 0.5))).contiguous()
    ref = torch.randn(B, C, h, w, generator=gen) * 0.5
    srcs = [torch.randn(B, C, h, w, generator=gen) * 0.5 for _ in range(V - 1)]
    warped = [OC.homo_warping(srcs[i], K[:, 0], K[:, i + 1], E[:, 0], E[:, i + 1], hyp, (h, w)) for i in range(V - 1)]
    got = R.forward(_cl(ref), [_cl(s) for s in srcs], cams, hyp, geom="proj", cost="variance_cvp")[0]
    _compare("forward cvp variance", got, OC.variance_cost(ref, warped).movedim(1, -1))
    w0 = R.forward(None, [_cl(s) for s in srcs], cams, hyp, geom="proj", cost="warp_only", ref_hw=(h, w))[0]
    _compare("forward cvp warp", w0, torch.stack(warped).movedim(2, -1))


@pytest.mark.parametrize("case", ["per_batch", "per_pixel", "narrow_source"])
def test_forward_matches_vis_oracle_groupcorr(case):
    """HOMOG geometry: OV.warp_volume + the 8-group correlation, per-batch and per-pixel planes and a source narrower than 21 texels."""
    from oracle import vismvsnet as OV
    B, V, C, h, w, D = 2, 3, 32, 16, 20, 5
    hs, ws = (10, 13) if case == "narrow_source" else (14, 22)
    K, Rm, t, dmin, dmax = _rig(B, V, h, w, hs, ws)
    interval = ((dmax - dmin) / (D - 1)).view(B, 1, 1, 1)
    cam_arr = [OV.fill_cam_array(K[:, i], Rm[:, i], t[:, i], dmin, interval.view(B)) for i in range(V)]
    cams = _homog_blocks(OV, cam_arr[0], cam_arr[1:])
    gen = torch.Generator().manual_seed(7)
    start = dmin.view(B, 1, 1, 1)
    if case == "per_pixel":
        start = start + 0.4 * torch.rand(B, 1, h, w, generator=gen)
    planes = start + interval * torch.arange(D, dtype=torch.float32).view(1, D, 1, 1)
    planes = planes.reshape(B, D).contiguous() if case != "per_pixel" else planes.contiguous()
    ref = torch.randn(B, C, h, w, generator=gen) * 0.5
    srcs = [torch.randn(B, C, hs, ws, generator=gen) * 0.5 for _ in range(V - 1)]
    ref_vol = ref.unsqueeze(2).repeat(1, 1, D, 1, 1)
    warped = [OV.warp_volume(srcs[i], cam_arr[0], cam_arr[i + 1], D, start, interval, 1.0, (h, w)) for i in range(V - 1)]
    want = torch.stack([OV.groupwise_correlation(ref_vol, wv, 8) for wv in warped]).movedim(2, -1)      # [n,B,D,h,w,8]
    got = R.forward(_cl(ref), [_cl(s) for s in srcs], cams, planes, geom="homog", cost="groupcorr")[0]
    assert tuple(got.shape) == tuple(want.shape)
    _compare(f"forward groupcorr {case}", got, want)
    w0 = R.forward(None, [_cl(s) for s in srcs], cams, planes, geom="homog", cost="warp_only", ref_hw=(h, w))[0]
    _compare(f"forward homog warp {case}", w0, torch.stack(warped).movedim(2, -1))


@pytest.mark.parametrize("geom,cost,per_pixel", [("proj", "variance", False), ("proj", "variance_cvp", True), ("homog", "groupcorr", True),
                                                 ("homog", "warp_only", False)])
def test_row_slab_equals_the_rows_of_the_whole_grid(geom, cost, per_pixel):
    """``forward(..., ref_y0=k)`` on rows [k, k + hs) is EXACTLY those rows of the whole-grid call."""
    whole, slab = G.slab_rig(geom, per_pixel, whole=True), G.slab_rig(geom, per_pixel)
    gen = torch.Generator().manual_seed(3)
    C = 32
    ref = torch.randn(2, G.SLAB_ROWS, G.A_REF[1], C, generator=gen)
    srcs = [torch.randn(2, *G.A_SRC, C, generator=gen) for _ in range(2)]
    y0, hs_ = G.SLAB_Y0, G.SLAB_H
    if per_pixel:
        assert torch.equal(slab["depth"], whole["depth"][:, :, y0:y0 + hs_])
    full = R.forward(ref, srcs, whole["cams"], whole["depth"], geom=geom, cost=cost, temp=0.7, ref_hw=whole["ref_hw"])
    part = R.forward(ref[:, y0:y0 + hs_].contiguous(), srcs, slab["cams"], slab["depth"], geom=geom, cost=cost, temp=0.7, ref_hw=slab["ref_hw"],
                     ref_y0=y0)
    assert torch.equal(part[0], full[0][..., y0:y0 + hs_, :, :])
    for a, b in zip(part[1:], full[1:]):
        assert torch.equal(a, b[..., y0:y0 + hs_, :])
    other = R.forward(ref[:, y0:y0 + hs_].contiguous(), srcs, slab["cams"], slab["depth"], geom=geom, cost=cost, temp=0.7, ref_hw=slab["ref_hw"])
    assert not torch.equal(other[0], part[0])                  # (ref_y0 matters on this rig)


@pytest.mark.parametrize("with_ref", [True, False])
def test_partial_sums_finished_on_the_host_equal_the_variance(with_ref):
    """``variance_partial`` = (sum f, sum f^2); finished with either rule it is the ``variance`` / ``variance_cvp`` volume.  Without
    reference features the sums run over the warped views alone: adding the reference's own terms gives the same."""
    rig = G.partial_rig()
    gen = torch.Generator().manual_seed(4)
    ref = torch.randn(2, *G.A_REF, 32, generator=gen) * 0.5
    srcs = [torch.randn(2, *G.A_SRC, 32, generator=gen) * 0.5 for _ in range(4)]
    kw = dict(geom="proj", ref_hw=G.A_REF)
    sums = R.forward(ref if with_ref else None, srcs, rig["cams"], rig["depth"], cost="variance_partial", **kw)[0]
    assert tuple(sums.shape) == (2, 2, G.A_D, *G.A_REF, 32)
    if not with_ref:
        r = ref.double().unsqueeze(1)
        sums = torch.stack((sums[0] + r, sums[1] + r ** 2))
    for rule in ("variance", "variance_cvp"):
        want = R.forward(ref, srcs, rig["cams"], rig["depth"], cost=rule, **kw)[0]
        got = R.variance_finish(sums, 5, rule)
        assert float((got - want).abs().max()) <= 1e-13 * max(1.0, float(want.abs().max())), rule


def test_fragile_is_empty_on_a_frontal_rig_and_small_on_the_turned_one():
    """Frontal cameras: nothing is fragile.  A camera turned by ~75 degrees (q_z crosses zero inside the image at a slant): some
    samples are, and fewer than the cap.  A sample with q_z == 0 because every term is zero is exempt (``fragile``'s docstring)."""
    from wild_deep_mvs_amd import ops
    B, V, h, w, hs, ws, D = 2, 3, 16, 24, 14, 26, 8
    K, Rm, t, dmin, dmax = _rig(B, V, h, w, hs, ws)
    proj = _proj(K, Rm, t)
    dv = dmin.view(B, 1) + (dmax - dmin).view(B, 1) * torch.arange(D).view(1, D) / (D - 1)
    cams = ops.proj_cams([proj[:, i] for i in range(1, V)], proj[:, 0])
    f = R.fragile(cams, dv, "proj", (h, w), (hs, ws))
    assert tuple(f.shape) == (V - 1, B, D, h, w)
    assert int(f[0].sum()) == 0, "the frontal view has fragile samples"
    share = float(f.any(dim=0).double().mean())
    print(f"[fragile] turned rig: {int(f[1].sum())} fragile samples, voxel share {share:.4f}", flush=True)
    assert int(f[1].sum()) > 0 and share <= G.FRAGILE_CAP
    rig = G.narrow_source_rig()
    fz = R.fragile(rig["cams"], rig["depth"], "homog", rig["ref_hw"], rig["src_hw"])
    assert int(fz[0, 1].sum()) == 0                            # q_z == 0 exactly: not fragile
    near = rig["cams"].clone()
    near[0, 1, 6] = 1.0
    near[0, 1, 8] = -10.5                                      # q_z = (x + 0.5) - 10.5: zero at x = 10 through cancellation
    fz = R.fragile(near, rig["depth"], "homog", rig["ref_hw"], rig["src_hw"])
    assert bool(fz[0, 1, :, :, 10].all()) and not bool(fz[0, 1, :, :, 11].any())


def test_every_gpu_rig_keeps_the_fragile_share_below_the_cap():
    """The condition tests/test_gpu_warp_fwd.py puts on its inputs, exercised here from the reference alone (D = 44 included)."""
    for name, rig in G.all_rigs():
        share = G.fragile_share(rig)
        assert share <= G.FRAGILE_CAP, (name, share)
        assert rig["cams"].dtype == torch.float32 and rig["depth"].dtype == torch.float32 and rig["cams"].shape[2] == 18


@pytest.mark.parametrize("mode", G.B_MODES)
@pytest.mark.parametrize("kernel", list(G.POLICY))
def test_zoom_rigs_take_the_staging_mode_they_name(kernel, mode):
    """Group B's cases against the box rule of csrc/warp_box.h restated on float64 corner projections, with the slack of the box 1/64
    texel larger and smaller; ZERO: the volume equals the one with that view's features set to zero."""
    rig, hm = G.check_zoom_rig(kernel, mode)
    print(f"[rig] {kernel} {mode}: [view][DIRECT, GEN, FAST, ZERO] = {hm.tolist()}", flush=True)
    if mode == "zero":
        gen = torch.Generator().manual_seed(2)
        ref = torch.randn(1, *G.B_REF, 32, generator=gen)
        srcs = [torch.randn(1, *rig["src_hw"], 32, generator=gen) for _ in range(4)]
        cost = "groupcorr" if kernel == "groupcorr" else "variance"
        a = R.forward(ref, srcs, rig["cams"], rig["depth"], geom=rig["geom"], cost=cost)[0]
        srcs[2] = torch.zeros_like(srcs[2])
        assert torch.equal(a, R.forward(ref, srcs, rig["cams"], rig["depth"], geom=rig["geom"], cost=cost)[0])


def test_range_rig_needs_the_split_it_is_named_for():
    """Group C's rig on the restated box rule: per view the share of (tile, chunk) blocks that do not fit falls when the chunk is
    shorter -- 12 planes, 6, 4, 2 for the quad-owner kernel's 16-texel box."""
    rig = G.range_rig(44)
    rig = dict(rig, cams=rig["cams"][:, :1].contiguous(), depth=rig["depth"][:1].contiguous())          # (item 0)
    share = {}
    for planes in (12, 6, 4, 2):
        share[planes] = []
        for v, first in enumerate((32, 32, 24)):              # (view 2 has left the 57-texel map by plane 32)
            sub = dict(rig, depth=rig["depth"][:, first:first + planes].contiguous(), cams=rig["cams"][v:v + 1])
            hm = G.staging_modes(sub, "quad_owner", ppd=planes)
            share[planes].append(float(hm[0, G.DIRECT]) / float(hm[0].sum()))
    print(f"[rig] range rig, planes 32.. (view 2: 24..): share of blocks on global taps per view {share}", flush=True)
    # (of the four tiles of the 5 x 9 reference, the ragged ones of a single column have narrower boxes: shares, not all or nothing)
    assert share[12][0] > 0.0 and share[6][0] == 0.0                       # view 0: halves fit
    assert share[6][1] > 0.0 and share[4][1] == 0.0                        # view 1: quarters fit
    assert share[4][2] > 0.0 and share[2][2] == 0.0                        # view 2: two planes fit
