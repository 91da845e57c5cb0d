"""pscv_warp_cost_rows -- the generic direct-gather kernel (csrc/warp_cost.hip), the quad kernel (warp_cost_quad.hip), the LDS-staged
quad-owner kernel (warp_cost_tiled.hip), the lane-owner kernel (warp_cost_lv.hip) and the staged group-correlation kernel
(warp_gc_lv.hip) -- each against the plain float64 reference of tests/_warp_bwd_ref.py (``forward``), on identical, already rounded
operands and hand-written camera blocks (tests/_warp_fwd_rigs.py): every cost mode and geometry at every storage type pair, the four
staging modes of the three staged kernels, the adaptive split of a plane range, and the edges of the host path (16 views, a narrow
source map, source maps of another size, row slabs, partial variance sums).

tests/test_gpu_warp_cost.py holds the kernels against EACH OTHER, bit for bit: that cannot see an error in the code they share
(sweep_index, make_taps, blend_taps, the box rules, the host dispatch).  This file is the independent reference for each of them.
tests/test_warp_fwd_ref_cpu.py pins the reference to the oracles and checks every rig used here without a GPU.

A case shows that the family it names ran: the staged kernels count their per-(block, view) staging modes into
``pscv_debug_wl_mode_hist`` (a launch that took another kernel leaves it at zero); the quad and generic kernels are selected by the
knobs that exclude the others, and leave the histogram at zero."""
import ctypes

import pytest
import torch

import _warp_bwd_ref as R
import _warp_fwd_rigs as G

pytestmark = pytest.mark.gpu

# The project's own tolerances for this comparison (test_gpu_warp_cost.py against the goldens: max_abs 3e-4, rel_l2 2e-4): both sides
# get the same rounded operands and the kernels accumulate in fp32, so 16-bit storage adds one output rounding and nothing else.
TOL_L2, TOL_ABS = 2e-4, 3e-4
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
ULP = {F16: 2.0 ** -11, BF16: 2.0 ** -8}
TYPE_PAIRS = [(F32, F32), (F16, F16), (BF16, BF16), (F16, F32), (BF16, F32)]      # (features, out): all with_warp_types<true> admits
TEMP = 0.7


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from wild_deep_mvs_amd import _lib as L, ops
    geom = {"proj": L.GEOM_PROJ, "homog": L.GEOM_HOMOG}
    cost = {"variance": L.COST_VARIANCE, "variance_cvp": L.COST_VARIANCE_CVP, "softmin": L.COST_SOFTMIN, "groupcorr": L.COST_GROUPCORR,
            "warp_only": L.COST_WARP_ONLY, "variance_partial": L.COST_VARIANCE_PARTIAL}
    fn = L.lib().pscv_debug_wl_mode_hist
    fn.argtypes, fn.restype = [ctypes.c_void_p], None
    return L, ops, geom, cost, fn


def _tname(dt):
    return str(dt).replace("torch.", "")


def _operands(seed, C, B, ref_hw, src_hw, n_src, tf):
    """Random features already rounded to their storage type, channels-last, on the CPU: ref, srcs."""
    gen = torch.Generator().manual_seed(seed)
    (h, w), (hs, ws) = ref_hw, src_hw
    ref = (torch.randn(B, h, w, C, generator=gen) * 0.5).to(tf)
    srcs = [(torch.randn(B, hs, ws, C, generator=gen) * 0.5).to(tf) for _ in range(n_src)]
    return ref, srcs


_CASES = {}      # (name, cost, C, feature type) -> operands, float64 volume, fragile voxels: one evaluation shared by all families


def _case(name, rig, cost, C, tf, seed=21, temp=TEMP):
    key = (name, cost, C, tf)
    if key not in _CASES:
        n, B = rig["cams"].shape[:2]
        ref, srcs = _operands(seed, C, B, rig["ref_hw"], rig["src_hw"], n, tf)
        want = R.forward(None if cost == "warp_only" else ref, srcs, rig["cams"], rig["depth"], geom=rig["geom"], cost=cost, temp=temp,
                         ref_hw=rig["ref_hw"], ref_y0=rig["ref_y0"])[0]
        frag = R.fragile(rig["cams"], rig["depth"], rig["geom"], rig["ref_hw"], rig["src_hw"], rig["ref_y0"]).any(dim=0)      # [B,D,h,w]
        share = float(frag.double().mean())
        # a condition on the INPUTS (from float64 alone; tests/test_warp_fwd_ref_cpu.py asserts it for every rig without a GPU)
        assert share <= G.FRAGILE_CAP, (name, share)
        _CASES[key] = (ref, srcs, want, frag)
    return _CASES[key]


def _launch(env, ref, srcs, rig, cost, out_dtype, knobs, temp=TEMP):
    """One launch under the tuning ``knobs`` with the staged kernels' mode histogram switched on -> (volume on the CPU, histogram
    [view][DIRECT, GEN, FAST, ZERO])."""
    L, ops, GEOM, COST, fn = env
    dev = lambda x: None if x is None else x.cuda()
    hist = torch.zeros(16, dtype=torch.int32, device="cuda")
    with L.tuning(**knobs):
        fn(hist.data_ptr())
        try:
            out = ops.warp_cost(dev(ref), [dev(s) for s in srcs], dev(rig["cams"]), dev(rig["depth"]), geom=GEOM[rig["geom"]],
                                cost=COST[cost], temp=temp, ref_hw=rig["ref_hw"], out_dtype=out_dtype, ref_y0=rig["ref_y0"])
            torch.cuda.synchronize()
        finally:
            fn(None)
    return out.cpu(), hist.view(4, 4).cpu().long()


def _check(name, got, want, frag, worst):
    """``got`` against the float64 volume over the voxels that are not fragile (those only have to be finite): relative L2 and a
    per-element bound --
    fp32 out: rel_l2 <= 2e-4, |got - want| <= 3e-4 scale; 16-bit out: rel_l2 <= ulp, |got - want| <= ulp |want| + 3e-4 scale,
    scale = max(1, max|want|), ulp = 2^-11 (fp16) / 2^-8 (bf16)."""
    out_dtype = got.dtype
    got = got.double()
    assert tuple(got.shape) == tuple(want.shape), (name, tuple(got.shape), tuple(want.shape))
    assert bool(torch.isfinite(got).all()), f"{name}: non-finite values"
    keep = ~(frag.unsqueeze(-1) if want.dim() == 5 else frag.unsqueeze(-1).unsqueeze(0))
    keep = keep.expand_as(want)
    g, w_ = got[keep], want[keep]
    scale = max(1.0, float(w_.abs().max()))
    if float(w_.norm()) == 0.0:
        rel = 0.0 if float(g.abs().max()) == 0.0 else float("inf")
    else:
        rel = float((g - w_).norm() / w_.norm())
    if out_dtype == F32:
        tol_l2, bound = TOL_L2, torch.full_like(w_, TOL_ABS * scale)
    else:
        tol_l2, bound = ULP[out_dtype], ULP[out_dtype] * w_.abs() + TOL_ABS * scale
    r_abs = float(((g - w_).abs() / bound).max())
    print(f"[warp fwd] {name}: rel_l2={rel:.3e} (tol {tol_l2:.1e}), max |err| / bound = {r_abs:.3f}, max_abs={float((g - w_).abs().max()):.3e}, "
          f"scale {scale:.3g}, fragile {int(frag.sum())} of {frag.numel()}", flush=True)
    worst.append(max(rel / tol_l2, r_abs))
    assert rel <= tol_l2, (name, rel, tol_l2)
    assert r_abs <= 1.0, (name, r_abs)


def _families(geom, cost, C, per_pixel, tf, to, n_src, src_hw):
    """(name, knobs, staged kernel or None) of every family pscv_warp_cost_rows admits for the call, by the rule the host code states:
    the specialised kernels take C = 32 in a 16-bit format with the output in the same format or fp32 (and no ``warp_lpv``
    override); the two variance sweeps PROJ with per-batch planes and at most four views (the lane-owner one not the soft-min); the
    staged group correlation HOMOG with the output in the input's format and a source map of at least 21 texels each way."""
    fams = [("generic", dict(warp_tiled=0, warp_q2=0), None)]
    if C == 32:
        fams += [(f"generic lpv {k}", dict(warp_lpv=k), None) for k in (4, 2, 1)]
    if C == 32 and tf in (F16, BF16) and to in (tf, F32):
        fams.append(("quad", dict(warp_tiled=0, warp_q2=1), None))
        if geom == "proj" and not per_pixel and n_src <= 4 and cost in ("variance", "variance_cvp", "softmin"):
            fams.append(("quad-owner", dict(warp_tiled=1, warp_gc_lds=0), "quad-owner"))
            if cost != "softmin":
                fams.append(("lane-owner", dict(warp_tiled=4), "lane-owner"))
                fams.append(("lane-owner, general path", dict(warp_tiled=4, warp_tile=7), "lane-owner"))
        if geom == "homog" and cost == "groupcorr" and to == tf and min(src_hw) >= 21:
            fams.append(("staged groupcorr", dict(warp_tiled=1, warp_gc_lds=2), "groupcorr"))
            fams.append(("staged groupcorr, nothing staged", dict(warp_tiled=1, warp_gc_lds=2, warp_tile=7), "groupcorr"))
    return fams


def _run_families(env, tag, rig, cost, C, tf, to, per_pixel=False, only=None):
    """Every admitted family (or those named in ``only``) on one case; returns {family: histogram}."""
    ref, srcs, want, frag = _case(tag.split(" | ")[0], rig, cost, C, tf)
    n = rig["cams"].shape[0]
    worst, hists, ran = [], {}, []
    for name, knobs, staged in _families(rig["geom"], cost, C, per_pixel, tf, to, n, rig["src_hw"]):
        if only is not None and name not in only:
            continue
        got, hm = _launch(env, None if cost == "warp_only" else ref, srcs, rig, cost, to, knobs)
        if staged:
            assert int(hm[:min(n, 4)].sum()) > 0, f"{tag} {name}: the staged kernel did not run (empty mode histogram)"
            if staged == "groupcorr" and knobs.get("warp_tile") == 7:      # (the lane-owner kernel's general path still stages)
                assert int(hm[:, G.GEN].sum() + hm[:, G.FAST].sum()) == 0, (name, hm.tolist())
        else:
            assert int(hm.sum()) == 0, f"{tag} {name}: a staged kernel ran instead ({hm.tolist()})"
        _check(f"{tag} {name}", got, want, frag, worst)
        hists[name] = hm
        ran.append(name)
    print(f"[warp fwd] {tag}: families {ran}: worst measured / tolerance = {max(worst):.3f}", flush=True)
    return hists


# ---- A. mode and type matrix ------------------------------------------------------------------------------------------------------
MATRIX_MODES = [("proj", "variance", 32, False), ("proj", "variance_cvp", 16, True), ("proj", "variance_cvp", 32, False),
                ("proj", "softmin", 32, False), ("proj", "warp_only", 32, False), ("proj", "warp_only", 16, False),
                ("homog", "groupcorr", 32, False), ("homog", "groupcorr", 32, True), ("homog", "warp_only", 32, False)]


@pytest.mark.parametrize("tf,to", TYPE_PAIRS, ids=[f"{_tname(a)}-{_tname(b)}" for a, b in TYPE_PAIRS])
@pytest.mark.parametrize("geom,cost,C,per_pixel", MATRIX_MODES, ids=[f"{g}-{c}-C{ch}{'-perpixel' if pp else ''}" for g, c, ch, pp in MATRIX_MODES])
def test_mode_and_type_matrix(env, geom, cost, C, per_pixel, tf, to):
    """Every (geometry, cost) pair of the forward at every storage type pair, B = 2 with different cameras and depth rows per item,
    one camera per item partly behind, reference 11 x 21, source 23 x 29, D = 6 -- through EVERY family that admits the call: generic
    (``warp_lpv`` 0 and, for 32 channels, 4 / 2 / 1), quad, staged quad-owner, lane-owner (fast and general path), staged group
    correlation (and with nothing staged).

    Worst measured / tolerance over the modes and families on MI355X, per type pair: fp32 output (from fp32, fp16 or bf16 features)
    0.015 -- rel_l2 at most 1.7e-6 against 2e-4, every family within 1 % of the others; fp16 / fp16 0.58, bf16 / bf16 0.88, where the
    output rounding is the whole error (rel_l2 = 0.42-0.43 ulp in every mode; a per-element error of half a spacing is ulp |want| at the
    bottom of a binade)."""
    rig = G.matrix_rig(geom, per_pixel)
    tag = f"A {geom} {cost} C{C}{' per-pixel' if per_pixel else ''} | {_tname(tf)}/{_tname(to)}"
    _run_families(env, tag, rig, cost, C, tf, to, per_pixel)


# ---- B. staging modes of the three staged kernels ---------------------------------------------------------------------------------
B_KERNELS = {"quad_owner": ("quad-owner", ("variance", "softmin")), "lane_owner": ("lane-owner", ("variance", "variance_cvp")),
             "groupcorr": ("staged groupcorr", ("groupcorr",))}
B_CASES = [(k, c, m) for k, (_, costs) in B_KERNELS.items() for c in costs for m in G.B_MODES]


def _assert_mode(mode, hm):
    """What the histogram of a group-B case must show for the view in question (tests/_warp_fwd_rigs.py ``check_zoom_rig`` asserts the
    same of the box rule restated on the host; the quad-owner kernel counts every swept plane range, so only the shares are compared)."""
    only = lambda v, m: int(hm[v, m]) == int(hm[v].sum()) > 0
    if mode == "fast":
        assert all(only(v, G.FAST) for v in range(4)), hm.tolist()
    elif mode == "gen":
        assert int(hm[1, G.GEN]) > 0 and int(hm[1, G.DIRECT]) == 0 and all(only(v, G.FAST) for v in (0, 2, 3)), hm.tolist()
    elif mode == "zero":
        assert only(2, G.ZERO) and all(only(v, G.FAST) for v in (0, 1, 3)), hm.tolist()
    elif mode == "too_large":
        assert all(int(hm[v, G.DIRECT]) > 0 for v in range(4)), hm.tolist()
    elif mode == "arena_full":
        assert int(hm[0, G.DIRECT]) == 0 and int(hm[3, G.DIRECT]) > 0, hm.tolist()
    else:
        assert only(3, G.DIRECT) and all(only(v, G.FAST) for v in (0, 1, 2)), hm.tolist()


@pytest.mark.parametrize("tf", [F16, BF16], ids=_tname)
@pytest.mark.parametrize("kernel,cost,mode", B_CASES, ids=[f"{k}-{c}-{m}" for k, c, m in B_CASES])
def test_staging_modes(env, kernel, cost, mode, tf):
    """FAST (everything inside), GEN (a shift that clips the boxes of the border tiles), ZERO (one view wholly outside: it contributes
    f = 0), and DIRECT for each of its three reasons -- the box exceeds the largest box, the arena is full although each box fits, a
    corner lies behind the camera -- in each of the three staged kernels, on the pure-zoom rig (reference 10 x 20, D = 5, four views,
    C = 32).  The histogram assertion is what makes a case mean what its name says.

    Worst measured / tolerance over modes and costs on MI355X (fp16 / bf16; the output rounding dominates): quad-owner 0.49 / 0.86,
    lane-owner 0.45 / 0.86, group correlation 0.46 / 0.82.  Every case showed the histogram it names."""
    rig = G.zoom_rig(kernel, mode)
    family = B_KERNELS[kernel][0]
    tag = f"B {kernel} {mode} {cost} | {_tname(tf)}"
    hm = _run_families(env, tag, rig, cost, 32, tf, tf, only=(family,))[family]
    print(f"[warp fwd] {tag}: histogram [view][DIRECT, GEN, FAST, ZERO] = {hm.tolist()}", flush=True)
    _assert_mode(mode, hm)


# ---- C. plane ranges --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [44, 5, 1])
def test_plane_ranges_and_adaptive_split(env, D):
    """Plane-dependent shifts of 0.8, 1.5 and 3 texels per plane (tests/_warp_fwd_rigs.py ``range_rig``): whole chunks whose boxes do
    not fit while their halves or quarters do.  D = 44 on 128 items of a 5 x 9 reference (512 tiles, the fewest at which the launch
    plan keeps 32 planes per workgroup): chunks of 32 and 12 planes (halves of 6, quarters of 4 + 2); D = 5 and 1 on a 16 x 24
    reference: chunks of 4 + 1 and 1 planes (halves of 2).  The quad-owner kernel at ``warp_tile`` 0 (halves and quarters), 3
    (halves) and 1 (no split), the lane-owner kernel at 0 and 2 (halves), ``warp_ppd`` overrides that give 6 or (small launches: halved
    to) 3 planes per workgroup, and the generic and quad kernels at 3 / 4: all against float64, variance, fp16.  Each split level
    must lower the share of (plane range, view) pairs on global taps where a chunk has more than one plane.

    Worst measured / tolerance on MI355X: D = 44 0.51, D = 5 0.52, D = 1 0.42.  Share on global taps at D = 44: quad-owner no split /
    halves / halves + quarters 0.74 / 0.34 / 0.17, lane-owner 0.39 -> 0.11 with halves."""
    rig = G.range_rig(D)
    tag = f"C D={D}"
    ref, srcs, want, frag = _case(tag, rig, "variance", 32, F16)
    runs = [("quad-owner, halves + quarters", dict(warp_tiled=1, warp_tile=0), True), ("quad-owner, halves", dict(warp_tiled=1, warp_tile=3), True),
            ("quad-owner, no split", dict(warp_tiled=1, warp_tile=1), True), ("lane-owner", dict(warp_tiled=4, warp_tile=0), True),
            ("lane-owner, halves", dict(warp_tiled=4, warp_tile=2), True), ("quad-owner, warp_ppd 6", dict(warp_tiled=1, warp_ppd=6), True),
            ("lane-owner, warp_ppd 6", dict(warp_tiled=4, warp_ppd=6), True), ("quad, warp_ppd 3", dict(warp_tiled=0, warp_q2=1, warp_ppd=3), False),
            ("generic, warp_ppd 3", dict(warp_tiled=0, warp_q2=0, warp_ppd=3), False)]
    worst, share = [], {}
    for name, knobs, staged in runs:
        got, hm = _launch(env, ref, srcs, rig, "variance", F16, knobs)
        assert (int(hm.sum()) > 0) == staged, (name, hm.tolist())
        if staged:
            share[name] = float(hm[:, G.DIRECT].sum()) / float(hm.sum())
            print(f"[warp fwd] {tag} {name}: histogram {hm.tolist()}, share on global taps {share[name]:.3f}", flush=True)
        _check(f"{tag} {name}", got, want, frag, worst)
    print(f"[warp fwd] {tag}: worst measured / tolerance = {max(worst):.3f}", flush=True)
    if D > 1:          # (D = 5: the 4-plane box of view 2 exceeds the quad-owner kernel's 16 texels, not the lane-owner kernel's 32)
        assert share["quad-owner, halves + quarters"] <= share["quad-owner, halves"] < share["quad-owner, no split"], share
    if D == 44:
        assert share["quad-owner, halves + quarters"] < share["quad-owner, halves"], share
        assert share["lane-owner, halves"] < share["lane-owner"], share


# ---- D. host-path edges -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tf,to", [(F16, F16), (BF16, F32), (F32, F32)], ids=["float16", "bfloat16-float32", "float32"])
def test_sixteen_source_views(env, tf, to):
    """16 source views, HOMOG group correlation, 12 x 16 reference, D = 3: the generic kernel's ray terms exceed the default 64 KiB of
    LDS (the dynamic-LDS opt-in of the launch helper); generic and quad.

    Worst measured / tolerance on MI355X: fp16 0.50, fp32 output 0.012."""
    _run_families(env, f"D 16 views | {_tname(tf)}/{_tname(to)}", G.many_views_rig(), "groupcorr", 32, tf, to, only=("generic", "quad"))


@pytest.mark.parametrize("cost", ["groupcorr", "warp_only"])
@pytest.mark.parametrize("tf", [F16, BF16, F32], ids=_tname)
def test_narrow_source_map(env, tf, cost):
    """HOMOG with a 9 x 15 source map: the grid clamp lies inside the border texel, so rays behind the camera carry a non-zero
    weight; one item of one view has q_z == 0 EXACTLY at every sample (behind: ``hz > 0``, not ``>=``).  Generic and quad; the staged
    group-correlation kernel, asked for, declines (source below 21 texels) and the quad kernel answers.

    Worst measured / tolerance on MI355X: fp16 0.45, bf16 0.87, fp32 0.007."""
    rig = G.narrow_source_rig()
    tag = f"D narrow source {cost} | {_tname(tf)}"
    _run_families(env, tag, rig, cost, 32, tf, tf, only=("generic", "quad"))
    if tf != F32:
        ref, srcs, want, frag = _case(tag.split(" | ")[0], rig, cost, 32, tf)
        got, hm = _launch(env, None if cost == "warp_only" else ref, srcs, rig, cost, tf, dict(warp_tiled=1, warp_gc_lds=2))
        assert int(hm.sum()) == 0, f"the staged kernel took a {rig['src_hw']} source map: {hm.tolist()}"
        _check(f"{tag} staged asked for, declined", got, want, frag, [])


@pytest.mark.parametrize("which", ["smaller", "larger"])
@pytest.mark.parametrize("tf", [F16, BF16, F32], ids=_tname)
def test_source_map_of_another_size(env, tf, which):
    """PROJ variance, three views, a 9 x 14 and a 31 x 40 source map under a 12 x 20 reference, every family.

    Worst measured / tolerance on MI355X: fp16 0.58, bf16 0.84, fp32 0.016."""
    _run_families(env, f"D {which} source | {_tname(tf)}", G.sized_source_rig(which), "variance", 32, tf, tf)


SLAB_CASES = {  # as test_row_slab_launch_equals_the_rows_of_the_whole_image_launch lists them; per-pixel planes where the family takes them
    "lds_variance": ("proj", "variance", 32, False, "quad-owner"), "lane_owner_variance": ("proj", "variance", 32, False, "lane-owner"),
    "quad_variance": ("proj", "variance", 32, False, "quad"), "quad_per_pixel": ("proj", "variance", 32, True, "quad"),
    "generic_16ch": ("proj", "variance_cvp", 16, True, "generic"), "homog_groupcorr": ("homog", "groupcorr", 32, True, "quad"),
    "homog_groupcorr_lds": ("homog", "groupcorr", 32, False, "staged groupcorr"),
    "homog_groupcorr_lds_per_pixel": ("homog", "groupcorr", 32, True, "staged groupcorr")}


@pytest.mark.parametrize("case", list(SLAB_CASES))
def test_row_slab_against_float64(env, case):
    """``ref_y0``: rows [3, 9) of a 13-row grid -- cropped reference map and per-pixel planes, the cameras of the whole grid -- against
    ``forward(..., ref_y0=3)``, one case per kernel family, fp16.

    Worst measured / tolerance on MI355X: 0.42-0.44 in all eight cases (the fp16 output rounding)."""
    geom, cost, C, per_pixel, family = SLAB_CASES[case]
    rig = G.slab_rig(geom, per_pixel)
    assert rig["ref_y0"] == G.SLAB_Y0 and rig["ref_hw"][0] == G.SLAB_H
    _run_families(env, f"D slab {case} | float16", rig, cost, C, F16, F16, per_pixel, only=(family,))


@pytest.mark.parametrize("tf", [F16, BF16, F32], ids=_tname)
def test_partial_variance_sums_and_finish(env, tf):
    """COST_VARIANCE_PARTIAL: four views split 2 + 2 over two launches, the first with the reference features and the second without;
    each launch's (sum f, sum f^2) and their sum against float64, then ``ops.variance_finish`` of the summed partials for both
    variance rules into both 16-bit types against the finish formulas applied to the float64 sums.

    Worst measured / tolerance on MI355X: the fp32 partial sums 0.011 (rel_l2 1.9e-6); finished into fp16 / bf16 0.83 / 0.86."""
    L, ops, GEOM, COST, fn = env
    rig = G.partial_rig()
    tag = f"D partial | {_tname(tf)}"
    ref, srcs, want_all, frag = _case("D partial", rig, "variance_partial", 32, tf)
    cams = rig["cams"]
    worst = []
    first = dict(rig, cams=cams[:2].contiguous())
    second = dict(rig, cams=cams[2:].contiguous())
    want1 = R.forward(ref, srcs[:2], first["cams"], rig["depth"], geom="proj", cost="variance_partial")[0]
    want2 = R.forward(None, srcs[2:], second["cams"], rig["depth"], geom="proj", cost="variance_partial", ref_hw=rig["ref_hw"])[0]
    assert float((want1 + want2 - want_all).abs().max()) <= 1e-12 * float(want_all.abs().max())
    got1, hm1 = _launch(env, ref, srcs[:2], first, "variance_partial", F32, {})
    got2, hm2 = _launch(env, None, srcs[2:], second, "variance_partial", F32, {})
    assert int(hm1.sum() + hm2.sum()) == 0
    _check(f"{tag} views 0-1 with ref", got1, want1, frag, worst)
    _check(f"{tag} views 2-3 without ref", got2, want2, frag, worst)
    total = got1 + got2
    _check(f"{tag} summed", total, want_all, frag, worst)
    for rule in ("variance", "variance_cvp"):
        want = R.variance_finish(want_all, 5, rule)
        for to in (F16, BF16):
            got = ops.variance_finish(total.cuda(), 5, cost=COST[rule], dtype=to).cpu()
            _check(f"{tag} finish {rule} -> {_tname(to)}", got, want, frag, worst)
    print(f"[warp fwd] {tag}: worst measured / tolerance = {max(worst):.3f}", flush=True)
