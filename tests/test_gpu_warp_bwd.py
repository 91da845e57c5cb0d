"""pscv_warp_cost_bwd (csrc/warp_bwd.hip: the LDS-privatised tiled kernel and the direct one-atomic-per-tap kernel) against the plain
float64 reference of tests/_warp_bwd_ref.py, on identical, already rounded operands: every cost mode and geometry, every storage
type pair, batches whose items differ, every box regime of the tiled kernel, the fixed-point contract, non-finite values and the
argument checks.  tests/test_warp_bwd_ref_cpu.py pins that reference to the oracle's autograd."""
import ctypes as C

import pytest
import torch

import _warp_bwd_ref as R

pytestmark = pytest.mark.gpu

# the project's own tolerances for this comparison (test_warp_cost_backward_fp32): both sides get the same rounded operands and
# accumulate in at least fp32, so 16-bit storage does not loosen them
TOL_FEATURE, TOL_TEMP = 2e-4, 1e-3
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
TYPE_PAIRS = [(F32, F32), (F16, F16), (BF16, BF16), (F16, F32), (BF16, F32)]      # (features, gradient): all with_warp_types<true> admits


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from wild_deep_mvs_amd import _lib as L, ops
    geom = {"proj": L.GEOM_PROJ, "homog": L.GEOM_HOMOG}
    cost = {"variance": L.COST_VARIANCE, "variance_cvp": L.COST_VARIANCE_CVP, "softmin": L.COST_SOFTMIN, "groupcorr": L.COST_GROUPCORR,
            "warp_only": L.COST_WARP_ONLY}
    return L, ops, geom, cost


def _tname(dt):
    return str(dt).replace("torch.", "")


def _operands(seed, cost, B, C, ref_hw, src_hw, D, n_src, tf, tg, g_sigma=0.1):
    """Random operands already rounded to their storage types, channels-last (CPU): ref (None for the plain warp), srcs, grad_out."""
    gen = torch.Generator().manual_seed(seed)
    (h, w), (hs, ws) = ref_hw, src_hw
    ref = (torch.randn(B, h, w, C, generator=gen) * 0.5).to(tf)
    srcs = [(torch.randn(B, hs, ws, C, generator=gen) * 0.5).to(tf) for _ in range(n_src)]
    shape = {"groupcorr": (n_src, B, D, h, w, C // 4), "warp_only": (n_src, B, D, h, w, C)}.get(cost, (B, D, h, w, C))
    g = (torch.randn(shape, generator=gen) * g_sigma).to(tg)
    return (None if cost == "warp_only" else ref), srcs, g


def _launch(env, ref, srcs, cams, depth, g, geom, cost, temp, ref_hw, direct):
    """One launch of the tiled (direct = 0) or the direct (1) kernel -> (dref, dsrcs, dtemp) on the CPU."""
    L, ops, GEOM, COST = env
    dev = lambda x: None if x is None else x.cuda()
    with L.tuning(warp_bwd_direct=direct):
        dref, dsrcs, dtemp = ops.warp_cost_bwd(dev(ref), [dev(s) for s in srcs], dev(cams), dev(depth.contiguous()), dev(g), geom=GEOM[geom],
                                               cost=COST[cost], temp=temp, ref_hw=ref_hw, want_dtemp=(cost == "softmin"))
        torch.cuda.synchronize()
    return (None if dref is None else dref.cpu()), [d.cpu() for d in dsrcs], (None if dtemp is None else dtemp.cpu())


def _close(name, got, want, tol, worst):
    """Relative L2 of a gradient tensor against the float64 reference (a reference that is identically zero asks for exact zeros)."""
    got, want = got.double(), want.double()
    assert bool(torch.isfinite(got).all()), name
    if float(want.abs().max()) == 0.0:
        rel = 0.0 if float(got.abs().max()) == 0.0 else float("inf")
    else:
        rel = float((got - want).norm() / want.norm())
    print(f"[warp bwd] {name}: rel_l2={rel:.3e} max_abs={float((got - want).abs().max()):.3e} (ref max {float(want.abs().max()):.3e})", flush=True)
    worst.append(rel / tol)
    assert rel <= tol, (name, rel, tol)


# The temperature gradient is ONE scalar: the sum of a signed term per voxel.  The kernels evaluate a term in fp32 with __expf of an
# argument near -10, i.e. to about 1e-6 of its size, so a relative tolerance of 1e-3 on the sum is a statement about the kernel only
# while sum|term| / |sum| stays below about 100 (1e-3 / 100 = ten times that precision).  Random operands whose terms cancel further
# than that (one seed in twenty does, to 1 part in 2400) are passed over: the condition is computed from the float64 reference alone.
MAX_TEMP_COND = 100.0
TEMP = 0.7


def _case(seed, cost, B, C, ref_hw, src_hw, D, n_src, tf, tg, cams, depth, geom):
    """Operands (first seed from ``seed`` on whose temperature gradient is well conditioned, see above) and their float64 reference."""
    for s in range(seed, seed + 8):
        ref, srcs, g = _operands(s, cost, B, C, ref_hw, src_hw, D, n_src, tf, tg)
        want = R.backward(ref, srcs, cams, depth, g, geom=geom, cost=cost, temp=TEMP, ref_hw=ref_hw)
        if cost != "softmin" or want["dtemp_cond"] <= MAX_TEMP_COND:
            if cost == "softmin":
                print(f"[warp bwd] soft-min operands: seed {s}, d temp = {float(want['dtemp']):.4g}, sum|term| / |sum| = {want['dtemp_cond']:.1f}", flush=True)
            return ref, srcs, g, want
    raise AssertionError("no well-conditioned soft-min operands in eight seeds")


def _compare_all(env, tag, ref, srcs, cams, depth, g, geom, cost, ref_hw, want, temp=TEMP):
    worst = []
    for direct in (0, 1):
        kn = "direct" if direct else "tiled"
        dref, dsrcs, dtemp = _launch(env, ref, srcs, cams, depth, g, geom, cost, temp, ref_hw, direct)
        for v, d in enumerate(dsrcs):
            _close(f"{tag} {kn}: d src{v}", d, want["dsrcs"][v], TOL_FEATURE, worst)
        if cost != "warp_only":
            _close(f"{tag} {kn}: d ref", dref, want["dref"], TOL_FEATURE, worst)
        if cost == "softmin":
            _close(f"{tag} {kn}: d temp", dtemp, want["dtemp"], TOL_TEMP, worst)
    print(f"[warp bwd] {tag}: worst measured / tolerance = {max(worst):.3f}", flush=True)
    return want


# ---- A. mode and type matrix ------------------------------------------------------------------------------------------------------
A_REF, A_SRC, A_D = (11, 21), (13, 23), 6       # two ragged 16 x 8 tiles each way; one full 4-plane chunk and a ragged one


def _matrix_rig(geom, per_pixel, seed=0):
    """Hand-written camera blocks [2 views, 2 items, 18] and depth rows that DIFFER between the two batch items.  View 0 is a mild
    affine map with a little perspective; view 1 has q_z = (1 - 0.08 x ...) crossing zero inside the reference image: the columns to
    its right lie behind that camera, the ones before it sweep through the source map and far out of it."""
    cams = torch.zeros(2, 2, 18)
    for b in range(2):
        cams[0, b, :12] = torch.tensor([1.04 + 0.03 * b, 0.03, 0.4, -0.02, 1.02 - 0.02 * b, 0.3 + 0.2 * b, 0.004, -0.003, 1.0,
                                        0.5 - 0.3 * b, -0.4, 0.05 * b])
        cams[1, b, :12] = torch.tensor([1.1, 0.02, 0.3, -0.03, 1.05, 0.2 + 0.1 * b, -0.08 - 0.01 * b, 0.0, 1.0,
                                        0.3, 0.2 * b, 0.02])
        if geom == "homog":                 # block[9:18] = Bm: hom = A p - (Bm p) / (d + 1e-9)
            cams[0, b, 9:] = torch.tensor([0.3, 0.0, 0.5 + 0.2 * b, 0.0, 0.2, -0.4, 0.001, 0.0, 0.03])
            cams[1, b, 9:] = torch.tensor([-0.2, 0.0, 0.4, 0.0, 0.1, 0.3 - 0.2 * b, 0.002, 0.0, -0.02])
    depth = torch.stack([torch.linspace(1.0, 2.0, A_D), torch.linspace(1.3, 2.6, A_D)])
    if per_pixel:
        gen = torch.Generator().manual_seed(100 + seed)
        depth = (depth.view(2, A_D, 1, 1) * (1.0 + 0.1 * (torch.rand(2, A_D, *A_REF, generator=gen) - 0.5))).contiguous()
    ix, iy, qz = R.positions(cams, depth, geom, A_REF, A_SRC)
    for b in range(2):                      # (checked on the CPU: without it the case would silently test something else)
        behind = float((qz[1, b] <= 0).double().mean())
        inside = float(((qz[1, b] > 0) & (ix[1, b] > 0) & (ix[1, b] < A_SRC[1] - 1) & (iy[1, b] > 0) & (iy[1, b] < A_SRC[0] - 1)).double().mean())
        assert 0.1 < behind < 0.9 and inside > 0.1, (geom, b, behind, inside)
        assert float((qz[0, b] > 0).double().mean()) == 1.0
    assert not torch.equal(cams[:, 0], cams[:, 1]) and not torch.equal(depth[0], depth[1])
    return cams, depth


MATRIX_MODES = [("proj", "variance", 32, False), ("proj", "variance_cvp", 16, True), ("proj", "softmin", 32, False),
                ("proj", "warp_only", 32, False), ("proj", "warp_only", 16, False), ("homog", "groupcorr", 32, False),
                ("homog", "groupcorr", 32, True), ("homog", "warp_only", 32, False)]


@pytest.mark.parametrize("tf,tg", TYPE_PAIRS, ids=[f"{_tname(a)}-{_tname(b)}" for a, b in TYPE_PAIRS])
@pytest.mark.parametrize("geom,cost,C,per_pixel", MATRIX_MODES, ids=[f"{g}-{c}-C{ch}{'-perpixel' if pp else ''}" for g, c, ch, pp in MATRIX_MODES])
def test_mode_and_type_matrix(env, geom, cost, C, per_pixel, tf, tg):
    """Every (geometry, cost) pair the backward has, at every storage type pair, B = 2 with different cameras and depth rows per item,
    one camera per item partly behind, both kernels: d ref, every d src and d temp against float64 autograd.

    Worst measured relative L2 over the five type pairs and both kernels on MI355X (tolerance 2e-4; d temp 1e-3):
    PROJ variance C32 2.0e-5 | PROJ CVP variance C16 per-pixel 2.2e-5 | PROJ soft-min C32 7.5e-6, d temp 8.7e-6 |
    PROJ plain warp C32 / C16 2.6e-6 | HOMOG group correlation per-batch / per-pixel 4.5e-6 | HOMOG plain warp 2.7e-6."""
    cams, depth = _matrix_rig(geom, per_pixel)
    ref, srcs, g, want = _case(11, cost, 2, C, A_REF, A_SRC, A_D, 2, tf, tg, cams, depth, geom)
    _compare_all(env, f"A {geom} {cost} C{C}{' per-pixel' if per_pixel else ''} {_tname(tf)}/{_tname(tg)}", ref, srcs, cams, depth, g, geom, cost, A_REF, want)


# ---- B. box regimes of the tiled kernel -------------------------------------------------------------------------------------------
B_REF, B_D = (10, 20), 5                         # a full 16 x 8 tile plus ragged ones; one full chunk of planes and a single plane
# zoom per regime: a 16 x 8 tile spreads over about (16 z + 2) x (8 z + 2) texels; capacity 512 texels at C = 32, 1024 at C = 16
B_ZOOM = {32: {"one": 1.0, "two": 2.2, "four": 3.4, "four_clipped": 7.0}, 16: {"one": 1.0, "two": 3.2, "four": 4.8, "four_clipped": 10.0}}
B_CASES = [(C, regime, cost) for C in (32, 16) for regime in ("one", "two", "four", "four_clipped")
           for cost in ("variance", "softmin", "groupcorr", "warp_only") if not (cost == "groupcorr" and C == 16)]


def _zoom_rig(geom, z, src_hw):
    """Pure scaling by z about the origin plus a sub-texel shift, two views.  PROJ: rot = diag(z, z, 1), trans = (tx, ty, 0), so the
    sample of pixel x on plane d is z x + tx / d.  HOMOG: A = the same with the zoom divided by the index scale (size - 1) / size and
    half-pixel centres, Bm = 0."""
    hs, ws = src_hw
    cams = torch.zeros(2, 1, 18)
    for v, (tx, ty) in enumerate(((0.37, 0.61), (0.71, 0.23))):
        if geom == "proj":
            cams[v, 0, :12] = torch.tensor([z, 0, 0, 0, z, 0, 0, 0, 1.0, tx, ty, 0.0])
        else:
            cams[v, 0, :9] = torch.tensor([z * ws / (ws - 1), 0, tx, 0, z * hs / (hs - 1), ty, 0, 0, 1.0])
    return cams, torch.linspace(1.0, 2.0, B_D).view(1, B_D)


@pytest.mark.parametrize("tf", [F16, F32], ids=_tname)
@pytest.mark.parametrize("C,regime,cost", B_CASES, ids=[f"C{c}-{r}-{k}" for c, r, k in B_CASES])
def test_box_regimes(env, C, regime, cost, tf):
    """One pass, two sub-passes, four sub-passes that fit, and four whose boxes still exceed the patch (clipped box + direct atomics),
    for the 512-texel patch of 32 channels and the 1024-texel patch of 16: the soft-min case has d ref and d temp, which a sub-pass
    must add exactly once per lane.  The rule of the kernel is restated on the host (R.box_regime) from the reference's sample
    positions and the case ASSERTS the regime it names, also with every box one texel larger and smaller.

    Worst measured relative L2 per regime over costs, types and both kernels on MI355X (tolerance 2e-4):
    C32 one 2.6e-5, two 2.0e-5, four 2.1e-5, four clipped 2.3e-5 | C16 one 2.4e-5, two 2.0e-5, four 2.0e-5, four clipped 2.5e-5;
    d temp (tolerance 1e-3) at most 1.6e-4, the tiled and the direct kernel within 2 % of each other's error."""
    geom = "homog" if cost == "groupcorr" else "proj"
    z = B_ZOOM[C][regime]
    src_hw = (int(B_REF[0] * z) + 3, int(B_REF[1] * z) + 3)          # just large enough for the zoomed reference image
    cams, depth = _zoom_rig(geom, z, src_hw)
    ix, iy, _ = R.positions(cams, depth, geom, B_REF, src_hw)
    for v in range(2):
        for grow in (-1, 0, 1):
            assert R.box_regime(ix[v, 0], iy[v, 0], src_hw, C, (0, 0), grow) == {regime}, (v, grow)
    ref, srcs, g, want = _case(12, cost, 1, C, B_REF, src_hw, B_D, 2, tf, tf, cams, depth, geom)
    _compare_all(env, f"B C{C} {regime} {cost} {_tname(tf)}", ref, srcs, cams, depth, g, geom, cost, B_REF, want)


# ---- C. fixed-point headroom, exact -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sign", [1.0, -1.0], ids=["pos", "neg"])
@pytest.mark.parametrize("tf", [F32, F16, BF16], ids=_tname)
@pytest.mark.parametrize("C", [32, 16])
def test_fixed_point_headroom_is_exact(env, C, tf, sign):
    """Plain warp with rot = 0, trans = (tx, ty, 1): every sample of every plane lands on ONE texel with weight exactly 1.  Reference
    16 x 32, D = 8: eight workgroups of 128 pixels x 4 planes per item and view, each adding 512 values just under 2^21 quanta -- the
    whole advertised headroom (9 bits for 512 adds).  The upstream gradient is the constant G just under 2 (all significand bits of
    the storage type set), so every partial sum is exactly representable: d src at that texel is 4096 G bit for bit and every other
    element is exactly zero, for the tiled and the direct kernel."""
    B, h, w, D, hs, ws = 2, 16, 32, 8, 9, 12
    G = sign * (2.0 - 2.0 ** -7 if tf == BF16 else 2.0 - 2.0 ** -10)
    target = {(0, 0): (5, 3), (0, 1): (7, 6), (1, 0): (0, 8), (1, 1): (11, 0)}      # (view, item) -> (tx, ty), corners included
    cams = torch.zeros(2, B, 18)
    for (v, b), (tx, ty) in target.items():
        cams[v, b, 9:12] = torch.tensor([float(tx), float(ty), 1.0])
    depth = torch.stack([torch.linspace(1.0, 2.0, D), torch.linspace(0.5, 3.0, D)])
    gen = torch.Generator().manual_seed(13)
    srcs = [torch.randn(B, hs, ws, C, generator=gen).to(tf) for _ in range(2)]
    g = torch.full((2, B, D, h, w, C), G).to(tf)
    assert float(g.float().flatten()[0]) == G
    for direct in (0, 1):
        _, dsrcs, _ = _launch(env, None, srcs, cams, depth, g, "proj", "warp_only", 0.0, (h, w), direct)
        for (v, b), (tx, ty) in target.items():
            want = torch.zeros(hs, ws, C)
            want[ty, tx] = D * h * w * G
            bad = int((dsrcs[v][b] != want).sum())
            print(f"[warp bwd] C headroom C{C} {_tname(tf)} G={G} {'direct' if direct else 'tiled'} view {v} item {b}: "
                  f"texel value {float(dsrcs[v][b][ty, tx, 0])!r} (want {D * h * w * G!r}), {bad} elements differ", flush=True)
            assert torch.equal(dsrcs[v][b], want), (direct, v, b, bad)


# ---- D. fixed-point resolution against the documented contract --------------------------------------------------------------------
def test_fixed_point_resolution_keeps_21_bits_below_the_bound(env):
    """Variance, fp32, ordinary random gradients plus ONE voxel per workgroup (tile x plane chunk) whose gradient is 2^10 times larger.
    Per texel of d src, |tiled - float64| <= taps(texel) q / 2 + 2^-20 sum|contribution|:
    * q = 2^(floor(log2 Bmax) - 20), Bmax = (2 / N) max|G| x 2 max|f| is the quantum the kernel documents ("21 bits below the bound are
      kept"), taken over the whole launch and so at least any workgroup's own; half a quantum per fixed-point add;
    * 2^-20 of the absolute sum is the allowance for the fp32 blend and for fp32 atomics in arbitrary order.
    Both terms come from R.tap_scatter.  The geometry has sample positions that fp32 holds EXACTLY (unit zoom, power-of-two depths,
    dyadic shifts: x + t / d), so the position arithmetic contributes nothing and the bound tests the accumulation alone: with
    ordinary positions one fp32 ulp of a position near 20 (2^-19 texels) times the outlier's gradient is as large as q / 2 itself.
    This catches a wrong scale, a wrong headroom and an overflow.

    Measured on MI355X (Bmax = 840, q = 4.9e-4, up to 24 taps per texel, the fixed-point term is > 99.9 % of the bound): largest
    error / bound 0.63 (view 0) and 0.98 (view 1).  What the ordinary gradients keep next to an outlier 2^10 times their size: d src
    as a whole is within 1.2e-4 / 1.3e-4 relative L2 of float64, against 2e-5 without the outliers (part A)."""
    B, C, D, n_src = 2, 32, 6, 2
    cams = torch.zeros(n_src, B, 18)
    for v in range(n_src):
        for b in range(B):
            cams[v, b, :12] = torch.tensor([1, 0, 0, 0, 1, 0, 0, 0, 1.0, 0.375 + 0.25 * v + 0.5 * b, 0.625 - 0.25 * v + 0.125 * b, 0.0])
    depth = torch.tensor([[1.0, 2.0, 4.0, 0.5, 8.0, 0.25], [2.0, 0.5, 1.0, 16.0, 0.25, 4.0]])
    ref, srcs, g = _operands(14, "variance", B, C, A_REF, A_SRC, D, n_src, F32, F32)
    gen = torch.Generator().manual_seed(15)
    for b in range(B):
        for ty in range(0, A_REF[0], R.TILE_H):
            for tx in range(0, A_REF[1], R.TILE_W):
                for d0 in range(0, D, R.TILE_PLANES):
                    y = ty + int(torch.randint(0, min(R.TILE_H, A_REF[0] - ty), (1,), generator=gen))
                    x = tx + int(torch.randint(0, min(R.TILE_W, A_REF[1] - tx), (1,), generator=gen))
                    d = d0 + int(torch.randint(0, min(R.TILE_PLANES, D - d0), (1,), generator=gen))
                    g[b, d, y, x] *= 1024.0
    want = R.backward(ref, srcs, cams, depth, g, geom="proj", cost="variance")
    ix32 = want["ix"].float().double()
    assert torch.equal(ix32, want["ix"]) and torch.equal(want["iy"].float().double(), want["iy"])       # positions exact in fp32
    q, bmax = R.fixed_point_quantum(g, [ref] + srcs, n_src)
    _, dsrcs, _ = _launch(env, ref, srcs, cams, depth, g, "proj", "variance", 0.0, A_REF, 0)
    worst = 0.0
    for v in range(n_src):
        taps, abs_sum, signed = R.tap_scatter(want["ix"][v], want["iy"][v], want["gw"][v], A_SRC)
        assert float((signed - want["dsrcs"][v]).abs().max()) <= 1e-9 * float(abs_sum.max())
        bound = taps.unsqueeze(-1).double() * (q / 2) + 2.0 ** -20 * abs_sum
        err = (dsrcs[v].double() - want["dsrcs"][v]).abs()
        assert bool((err[bound == 0] == 0).all())
        ratio = float((err / bound.clamp(min=1e-300)).max())
        rel = float((dsrcs[v].double() - want["dsrcs"][v]).norm() / want["dsrcs"][v].norm())
        share = float((taps.unsqueeze(-1).double() * (q / 2)).expand_as(bound).sum() / bound.sum())
        print(f"[warp bwd] D resolution view {v}: Bmax={bmax:.4g} q={q:.3e} max error / bound = {ratio:.3f}, rel_l2={rel:.3e}, "
              f"max taps per texel {int(taps.max())}, fixed-point share of the bound {share:.3f}", flush=True)
        worst = max(worst, ratio)
    assert worst <= 1.0, worst


# ---- E. non-finite values are not swallowed ---------------------------------------------------------------------------------------
E_CASES = [(cost, value, place) for cost in ("variance", "warp_only") for value in (float("nan"), float("inf"))
           for place in ("grad", "src", "ref") if not (cost == "warp_only" and place == "ref")]      # the plain warp takes no reference features


@pytest.mark.parametrize("cost,value,place", E_CASES, ids=[f"{c}-{v}-in-{p}" for c, v, p in E_CASES])
def test_non_finite_values_reach_the_output(env, cost, value, place):
    """One NaN or +inf in the upstream gradient of a single voxel, in a single source feature value or in a single reference feature
    value (fp16, both kernels): every d src / d ref element that is non-finite in float64 autograd and has a tap of non-zero weight
    is non-finite here, and nothing that is finite there is non-finite here.  The finite rest still matches the reference.  (The
    poisoned texel and voxel are interior: a border texel is also read, with weight zero, by samples outside the map.)"""
    cams, depth = _matrix_rig("proj", False)
    ref, srcs, g = _operands(16, cost, 2, 32, A_REF, A_SRC, A_D, 2, F16, F16)
    if place == "grad":
        if cost == "warp_only":
            g[0, 1, 2, 4, 5, 7] = value          # view 0, item 1, plane 2, pixel (4, 5): in front of both cameras, inside the map
        else:
            g[1, 2, 4, 5, 7] = value
    elif place == "src":
        srcs[0][1, 6, 4, 3] = value           # an interior texel that pixels in front of BOTH cameras sample
    else:
        ref[0, 3, 6, 20] = value
    want = R.backward(ref, srcs, cams, depth, g, geom="proj", cost=cost, ref_hw=A_REF)
    n_bad_ref = sum(int((~torch.isfinite(d)).sum()) for d in want["dsrcs"])
    # (the plain warp's gradient does not depend on the feature values at all: a poisoned source feature must leave it finite)
    assert (n_bad_ref > 0) == (not (cost == "warp_only" and place == "src"))
    for direct in (0, 1):
        kn = "direct" if direct else "tiled"
        dref, dsrcs, _ = _launch(env, ref, srcs, cams, depth, g, "proj", cost, 0.0, A_REF, direct)
        pairs = [(f"d src{v}", dsrcs[v], want["dsrcs"][v], R.tap_scatter(want["ix"][v], want["iy"][v], torch.ones_like(want["gw"][v]), A_SRC)[0] > 0)
                 for v in range(2)]
        if cost != "warp_only":
            pairs.append(("d ref", dref, want["dref"], torch.ones(dref.shape[:3], dtype=torch.bool)))
        for name, got, exp, touched in pairs:
            bad_exp = ~torch.isfinite(exp) & touched.unsqueeze(-1)
            bad_got = ~torch.isfinite(got)
            lost = int((bad_exp & ~bad_got).sum())
            extra = int((bad_got & torch.isfinite(exp)).sum())
            print(f"[warp bwd] E {cost} {value} in {place} {kn} {name}: {int(bad_exp.sum())} non-finite expected, {int(bad_got.sum())} got, "
                  f"{lost} swallowed, {extra} spurious", flush=True)
            assert lost == 0 and extra == 0, (kn, name, lost, extra)
            ok = torch.isfinite(exp) & ~bad_got
            rel = float((got.double()[ok] - exp[ok]).norm() / exp[ok].norm())
            assert rel <= TOL_FEATURE, (kn, name, rel)


# ---- F. refused, not launched -----------------------------------------------------------------------------------------------------
def _refused_cases(L):
    return [
        ("homog_variance", dict(geom=L.GEOM_HOMOG, cost=L.COST_VARIANCE), f"cost mode {L.COST_VARIANCE} is not available with geometry {L.GEOM_HOMOG}"),
        ("groupcorr_c16", dict(geom=L.GEOM_HOMOG, cost=L.COST_GROUPCORR, C=16), f"cost mode {L.COST_GROUPCORR} is not available with geometry {L.GEOM_HOMOG}"),
        ("c8", dict(C=8), "unsupported channel count C=8"),
        ("f16_features_bf16_grad", dict(tf=F16, tg=BF16), f"unsupported dtype pair in={L.F16} grad={L.BF16}"),
        ("f32_features_f16_grad", dict(tf=F32, tg=F16), f"unsupported dtype pair in={L.F32} grad={L.F16}"),
        ("n_src_0", dict(n_src=0), "n_src=0 outside [1,"),
        ("hs_1", dict(hs=1), "hs=1"),
    ]


@pytest.mark.parametrize("case", ["homog_variance", "groupcorr_c16", "c8", "f16_features_bf16_grad", "f32_features_f16_grad", "n_src_0", "hs_1"])
@pytest.mark.parametrize("direct", [0, 1], ids=["tiled", "direct"])
def test_refused_before_any_launch(env, direct, case):
    """Argument checks of pscv_warp_cost_bwd: PscvError naming the argument, the outputs untouched (they hold a sentinel)."""
    L, ops, GEOM, COST = env
    _, kw, reason = next(c for c in _refused_cases(L) if c[0] == case)
    geom, cost, Cc = kw.get("geom", L.GEOM_PROJ), kw.get("cost", L.COST_VARIANCE), kw.get("C", 32)
    tf, tg, n_src, hs = kw.get("tf", F16), kw.get("tg", F16), kw.get("n_src", 2), kw.get("hs", 9)
    code = {F32: L.F32, F16: L.F16, BF16: L.BF16}
    B, h, w, ws, D = 1, 8, 16, 12, 4
    ref = torch.zeros(B, h, w, Cc, dtype=tf, device="cuda")
    srcs = [torch.zeros(B, max(hs, 2), ws, Cc, dtype=tf, device="cuda") for _ in range(2)]
    cams = torch.zeros(2, B, 18, device="cuda")
    cams[:, :, 0] = cams[:, :, 4] = cams[:, :, 8] = 1.0
    depth = torch.ones(B, D, device="cuda")
    g = torch.zeros(2, B, D, h, w, Cc, dtype=tg, device="cuda")               # large enough for every output layout
    dref = torch.full((B, h, w, Cc), 7.0, device="cuda")
    dsrcs = [torch.full((B, max(hs, 2), ws, Cc), 7.0, device="cuda") for _ in range(2)]
    dtemp = torch.full((1,), 7.0, device="cuda")
    sp = (C.c_void_p * 2)(*[s.data_ptr() for s in srcs])
    dp = (C.c_void_p * 2)(*[s.data_ptr() for s in dsrcs])
    with L.tuning(warp_bwd_direct=direct):
        rc = L.lib().pscv_warp_cost_bwd(ref.data_ptr(), sp, n_src, cams.data_ptr(), depth.data_ptr(), depth.stride(0), 0, geom, cost, 0.5,
                                        g.data_ptr(), dref.data_ptr(), dp, dtemp.data_ptr(), B, Cc, h, w, hs, ws, D, code[tf], code[tg],
                                        ops._stream())
        with pytest.raises(L.PscvError) as ei:
            L.check(rc, "pscv_warp_cost_bwd")
    torch.cuda.synchronize()
    print(f"[warp bwd] F {case}: {ei.value}", flush=True)
    assert rc == -1 and "pscv_warp_cost_bwd" in str(ei.value) and reason in str(ei.value), str(ei.value)
    for out in [dref, dtemp] + dsrcs:
        assert bool((out == 7.0).all()), case
