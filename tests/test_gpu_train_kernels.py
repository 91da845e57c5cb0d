"""The training kernels of csrc/train_elem.hip, csrc/fuse.hip and csrc/conv3d_wgrad.hip against the float64 restatements of
tests/_train_ref.py, at the shapes where such kernels go wrong: a single partial block, ragged chunk counts, a second
grid-stride step, group counts that do not divide the workspace, a workgroup that carries its accumulators over several
tiles, padded channel tiles, channel slices.  Every kernel gets two kinds of input:

(a) EXACT inputs -- small integers, power-of-two scales, half-integer biases -- for which every product and partial sum is
    exact in fp32 and every result exact in bf16 and fp16 (tests/test_train_ref_cpu.py checks that on these very inputs).
    Any summation order gives the same bits: the assertion is torch.equal, with no tolerance to hide a wrong tail, carry,
    group or tap behind.
(b) REAL inputs (randn rounded to the storage type), element-wise against float64:
        16-bit output      |got - ref| <= ulp16(ref) / 2 + K 2^-24 T
        fp32 reduction     |got - ref| <= K 2^-24 A
    T / A = the float64 sum of the absolute values of the expression's terms, K = the number of fp32 roundings of one output
    (element-wise kernels) or the longest chain of dependent fp32 additions (reductions), counted next to each assertion.
    The kernels built on __expf / __logf / expf (softmax heads, fusion) have no derivable K: theirs is measured (the worst
    (|got - ref| - ulp16 / 2) / (2^-24 T) is printed by every test) and the bound is four times the worst measurement,
    rounded up to a power of two; profiles/train_kernels_precision.txt records measurements and bounds.
"""
import math

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import _train_ref as R

pytestmark = pytest.mark.gpu
U32 = R.U32


# ---- assertions --------------------------------------------------------------------------------------------------------------------
def host(x):
    return x.detach().to("cpu", torch.float64)


def assert_bits(name, got, ref, dtype=None):
    """torch.equal of the kernel's output with the float64 reference (rounded to the storage type when one is given)."""
    got, ref = host(got), (ref if dtype is None else R.round16(ref, dtype))
    if not torch.equal(got, ref.reshape(got.shape)):
        bad = got != ref.reshape(got.shape)
        i = torch.nonzero(bad)[0].tolist()
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} elements differ; first at {i}: got {float(got[tuple(i)])!r}, "
                             f"ref {float(ref.reshape(got.shape)[tuple(i)])!r}")


def ratio(got, ref, T, dtype=None, skip=None):
    """Worst (|got - ref| - ulp16(ref) / 2) / (2^-24 T) over the tensor (no ulp term for an fp32 output); inf for a NaN or where a
    bound of zero is exceeded."""
    got, ref, T = host(got), ref.reshape(got.shape), T.reshape(got.shape)
    excess = (got - ref).abs() - (R.ulp16(ref, dtype) / 2 if dtype is not None else 0.0)
    r = torch.where(excess > 0, excess / (U32 * T), torch.zeros_like(excess))
    r = torch.where(torch.isnan(excess), torch.full_like(r, math.inf), r)
    if skip is not None:
        r = r[~skip]
    return float(r.max()) if r.numel() else 0.0


def assert_within(name, got, ref, T, K, dtype=None, excused=None):
    """|got - ref| <= [ulp16(ref) / 2 +] K 2^-24 T element-wise; ``excused``: a mask of at most 1e-5 of the tensor left out.  Prints
    the worst ratio before it asserts."""
    got, ref, T = host(got), ref.reshape(got.shape), T.reshape(got.shape)
    tol = K * U32 * T + (R.ulp16(ref, dtype) / 2 if dtype is not None else 0.0)
    bad = ~((got - ref).abs() <= tol)                  # (a NaN fails)
    if excused is not None:
        excused = excused.reshape(got.shape)
        assert int(excused.sum()) <= 1e-5 * excused.numel(), f"{name}: {int(excused.sum())} excused elements"
        bad &= ~excused
    print(f"[precision] {name}: worst ratio {ratio(got, ref, T, dtype, excused):.4g} (bound K = {K:g})", flush=True)
    if bad.any():
        i = tuple(torch.nonzero(bad)[0].tolist())
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} elements outside the bound; first at {i}: got {float(got[i])!r}, "
                             f"ref {float(ref[i])!r}, tolerance {float(tol[i]):.3e}")


def bn_gpu(c, groups):
    """The case's tensors on the GPU; per-group constants as rows of the [G,4,C] / [G,5,C] tensors (plain form: [C] vectors)."""
    fin, co = c["fin"].cuda(), c["co"].cuda()
    row = (lambda t, k: t[0, k].contiguous()) if groups == 1 else (lambda t, k: t[:, k])
    return dict(y=c["y"].cuda(), dact=c["dact"].cuda(), skip=c["skip"].cuda(), scale=row(fin, 0), bias=row(fin, 1),
                ca=row(co, 0), cb=row(co, 1), cc=row(co, 2))


def cpu_rows(c):
    return c["fin"][:, 0], c["fin"][:, 1], c["co"][:, 0], c["co"][:, 1], c["co"][:, 2]


# =======================================================================================================================
# reductions: bn_stats, bn_bwd_reduce, relu_bwd_sum
# =======================================================================================================================
@pytest.mark.parametrize("dtype", R.DT)
@pytest.mark.parametrize("C,nvox,groups", R.BN_SMALL + [R.RED_MULTI] + R.RED_GROUPED)
def test_reductions_exact(C, nvox, groups, dtype):
    """Integer inputs: the per-channel sums are the float64 sums bit for bit at every geometry -- one partial block with idle lanes
    (3 voxels), ragged chunk counts (777), a second grid-stride step of all 1024 blocks (RED_MULTI), and 2 / 5 / 256 groups with
    1024 // groups blocks each taking two or more steps.  A group of zeros sums to exactly 0: nothing leaks between groups."""
    from wild_deep_mvs_amd import ops
    c = R.bn_case(C, nvox, groups, dtype, True)
    if groups > 1:
        c["y"][1] = 0
        c["dact"][1] = 0
    d = bn_gpu(c, groups)
    sc, bi = c["fin"][:, 0], c["fin"][:, 1]
    sums = ops.bn_stats(d["y"], groups)
    assert_bits("bn_stats", sums.reshape(groups, 2, C), R.bn_sums(c["y"], groups))
    for relu in (False, True):
        s = ops.bn_bwd_reduce(d["dact"], d["y"], d["scale"], d["bias"], relu=relu)
        assert_bits(f"bn_bwd_reduce relu={relu}", s.reshape(groups, 2, C), R.bn_bwd_sums(c["dact"], c["y"], sc, bi, relu))
        if groups > 1:
            assert float(s[1].abs().max()) == 0.0 and float(sums[1].abs().max()) == 0.0
    for slope in (0.0, 0.5):       # out = y: zeros included, they take the slope branch
        dpre, ssum = ops.relu_bwd_sum(d["dact"], d["y"], slope)
        rd, rs, rsum = R.relu_bwd(c["dact"], c["y"], slope, dtype)
        assert_bits(f"relu_bwd_sum slope={slope}: dpre", dpre, rd)
        assert_bits(f"relu_bwd_sum slope={slope}: sums", ssum, rsum)


@pytest.mark.parametrize("dtype", R.DT)
@pytest.mark.parametrize("C,nvox,groups", R.BN_SMALL + [R.RED_MULTI] + R.ELEM_GROUPED)
def test_reductions_real(C, nvox, groups, dtype):
    """|sum - ref| <= K 2^-24 A with A the sum of absolute values and K = the longest chain of dependent fp32 additions, counted
    by _train_ref.red_chain from the geometry the launch takes: the lane's grid-stride steps, the 256 / CG lanes of a channel
    group in block_reduce2, the finishing kernel's rows.  (Products of 16-bit values are exact in fp32 and enter through a fused
    multiply-add: no rounding of their own.)"""
    from wild_deep_mvs_amd import ops
    c = R.bn_case(C, nvox, groups, dtype, False)
    d = bn_gpu(c, groups)
    sc, bi = c["fin"][:, 0], c["fin"][:, 1]
    K = R.red_chain(nvox * (C // 8), groups, C // 8)
    assert_within("bn_stats", ops.bn_stats(d["y"], groups), R.bn_sums(c["y"], groups), R.bn_sums(c["y"], groups, absolute=True), K)
    # ReLU: an element whose z lies within fp32 rounding of zero may be counted on either side -- excused, its terms added to the bound
    near = R.relu_near_zero(c["y"], sc, bi)
    assert int(near.sum()) <= 1e-5 * near.numel()
    slack = R.bn_bwd_sums(torch.where(near, c["dact"].double(), 0.0), c["y"], sc, bi, False, absolute=True)
    for relu in (False, True):
        A = R.bn_bwd_sums(c["dact"], c["y"], sc, bi, relu, absolute=True) + (slack / (K * U32) if relu else 0.0)
        assert_within(f"bn_bwd_reduce relu={relu}", ops.bn_bwd_reduce(d["dact"], d["y"], d["scale"], d["bias"], relu=relu),
                      R.bn_bwd_sums(c["dact"], c["y"], sc, bi, relu), A, K)
    if groups == 1:
        dpre, ssum = ops.relu_bwd_sum(d["dact"], d["y"], 0.1)
        rd, _, _ = R.relu_bwd(c["dact"], c["y"], 0.1, dtype)
        assert_within("relu_bwd_sum slope=0.1: dpre", dpre, rd, rd.abs(), 1, dtype)        # K = 1: one multiplication
        stored = host(dpre).reshape(-1, C)                                                 # the header: the sum of what was STORED
        assert_within("relu_bwd_sum slope=0.1: sums", ssum, stored.sum(0), stored.abs().sum(0), K)


# =======================================================================================================================
# element-wise passes: bn_act, bn_bwd_apply, relu_bwd
# =======================================================================================================================
ACT_VARIANTS = [(relu, skip) for relu in (False, True, "post") for skip in (False, True)]


@pytest.mark.parametrize("dtype", R.DT)
@pytest.mark.parametrize("C,nvox,groups", R.BN_SMALL + R.ELEM_GROUPED)
def test_elementwise_exact(C, nvox, groups, dtype):
    """Integer volumes, scales +-{1, 2}, biases k + 0.5 (z is never 0, its sign is exact): every output element is the float64
    value bit for bit -- a lane on the wrong channel group, a wrong group offset or a missed tail chunk changes bits."""
    from wild_deep_mvs_amd import ops
    c = R.bn_case(C, nvox, groups, dtype, True)
    d = bn_gpu(c, groups)
    sc, bi, ca, cb, cc = cpu_rows(c)
    for relu, skip in ACT_VARIANTS:
        got = ops.bn_act(d["y"], d["scale"], d["bias"], relu=relu, skip=d["skip"] if skip else None)
        assert_bits(f"bn_act relu={relu} skip={skip}", got, R.bn_act(c["y"], sc, bi, relu, c["skip"] if skip else None)[0])
    for relu in (False, True):
        got = ops.bn_bwd_apply(d["dact"], d["y"], d["scale"], d["bias"], d["ca"], d["cb"], d["cc"], relu=relu)
        assert_bits(f"bn_bwd_apply relu={relu}", got, R.bn_bwd_apply(c["dact"], c["y"], sc, bi, ca, cb, cc, relu)[0])
    for slope in (0.0, 0.5):       # out = y holds exact zeros: they take the slope branch (gradient 0 for the ReLU)
        assert_bits(f"relu_bwd slope={slope}", ops.relu_bwd(d["dact"], d["y"], slope), R.relu_bwd(c["dact"], c["y"], slope, dtype)[0])
    assert int((c["y"] == 0).sum()) > 0


@pytest.mark.parametrize("dtype", R.DT)
def test_relu_branches_at_exact_zero(dtype):
    """z = y * scale + bias exactly 0 (integer bias here): the ReLU stores 0 and the backward takes the zero branch, dz = 0, in the
    reduction and in the apply pass alike -- `z > 0` on both sides, not `z >= 0`."""
    from wild_deep_mvs_amd import ops
    C, nvox = 16, 777
    c = R.bn_case(C, nvox, 1, dtype, True)
    c["fin"][:, 1] = torch.randint(-3, 4, (1, C), generator=R.gen(5)).float()
    d = bn_gpu(c, 1)
    sc, bi, ca, cb, cc = cpu_rows(c)
    z = R.f64(c["y"]).reshape(-1, C) * R.f64(sc) + R.f64(bi)
    assert int((z == 0).sum()) > 100 and float(R.f64(c["dact"]).reshape(-1, C)[z == 0].abs().sum()) > 0
    for relu in (True, "post"):
        assert_bits(f"bn_act relu={relu}", ops.bn_act(d["y"], d["scale"], d["bias"], relu=relu, skip=d["skip"]),
                    R.bn_act(c["y"], sc, bi, relu, c["skip"])[0])
    assert_bits("bn_bwd_reduce", ops.bn_bwd_reduce(d["dact"], d["y"], d["scale"], d["bias"], relu=True), R.bn_bwd_sums(c["dact"], c["y"], sc, bi, True)[0])
    assert_bits("bn_bwd_apply", ops.bn_bwd_apply(d["dact"], d["y"], d["scale"], d["bias"], d["ca"], d["cb"], d["cc"], relu=True),
                R.bn_bwd_apply(c["dact"], c["y"], sc, bi, ca, cb, cc, True)[0])


@pytest.mark.parametrize("dtype", R.DT)
def test_elementwise_exact_second_grid_stride_step(dtype):
    """Just above 8192 * 256 chunks and ragged: every block of the element-wise kernels visits a second chunk, where 'a lane keeps
    its channel group for its whole walk' is what makes its register-held constants the right ones."""
    from wild_deep_mvs_amd import ops
    C, nvox, groups = R.ELEM_MULTI
    c = R.bn_case(C, nvox, groups, dtype, True)
    d = bn_gpu(c, groups)
    sc, bi, ca, cb, cc = cpu_rows(c)
    assert_bits("bn_act relu=post + skip", ops.bn_act(d["y"], d["scale"], d["bias"], relu="post", skip=d["skip"]),
                R.bn_act(c["y"], sc, bi, "post", c["skip"])[0])
    assert_bits("bn_act relu=True", ops.bn_act(d["y"], d["scale"], d["bias"], relu=True), R.bn_act(c["y"], sc, bi, True)[0])
    assert_bits("bn_bwd_apply relu=True", ops.bn_bwd_apply(d["dact"], d["y"], d["scale"], d["bias"], d["ca"], d["cb"], d["cc"], relu=True),
                R.bn_bwd_apply(c["dact"], c["y"], sc, bi, ca, cb, cc, True)[0])
    assert_bits("relu_bwd slope=0.5", ops.relu_bwd(d["dact"], d["y"], 0.5), R.relu_bwd(c["dact"], c["y"], 0.5, dtype)[0])


@pytest.mark.parametrize("dtype", R.DT)
@pytest.mark.parametrize("C,nvox,groups", R.BN_SMALL + R.ELEM_GROUPED)
def test_elementwise_real(C, nvox, groups, dtype):
    from wild_deep_mvs_amd import ops
    c = R.bn_case(C, nvox, groups, dtype, False)
    d = bn_gpu(c, groups)
    sc, bi, ca, cb, cc = cpu_rows(c)
    near = R.relu_near_zero(c["y"], sc, bi)
    for relu, skip in ACT_VARIANTS:
        got = ops.bn_act(d["y"], d["scale"], d["bias"], relu=relu, skip=d["skip"] if skip else None)
        ref, T = R.bn_act(c["y"], sc, bi, relu, c["skip"] if skip else None)
        # K = 2 fp32 roundings: fma(y, scale, bias), the skip add (the ReLU selects, it does not round)
        assert_within(f"bn_act relu={relu} skip={skip}", got, ref, T, 2, dtype, excused=near if relu is True else None)
    for relu in (False, True):
        got = ops.bn_bwd_apply(d["dact"], d["y"], d["scale"], d["bias"], d["ca"], d["cb"], d["cc"], relu=relu)
        ref, T = R.bn_bwd_apply(c["dact"], c["y"], sc, bi, ca, cb, cc, relu)
        # K = 2 fp32 roundings: fma(cb, y, cc), then fma(ca, dz, .)
        assert_within(f"bn_bwd_apply relu={relu}", got, ref, T, 2, dtype, excused=near if relu else None)
    ref = R.relu_bwd(c["dact"], c["y"], 0.1, dtype)[0]
    assert_within("relu_bwd slope=0.1", ops.relu_bwd(d["dact"], d["y"], 0.1), ref, ref.abs(), 1, dtype)      # K = 1: one multiplication


# =======================================================================================================================
# [C]-vector bookkeeping: bn_finalize, bn_bwd_coeffs
# =======================================================================================================================
def _bn_module(C, affine, eps, momentum, g):
    bn = nn.BatchNorm3d(C, affine=affine, eps=eps, momentum=momentum).train()
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(C, generator=g)); bn.running_var.copy_(torch.rand(C, generator=g) + 0.5)
        if affine:
            bn.weight.copy_(torch.rand(C, generator=g) + 0.5); bn.bias.copy_(torch.randn(C, generator=g) * 0.3)
    return bn


def _finalize_bounds(sums, n, bn, eps, momentum, run0):
    """Reference and element-wise fp32 error bounds of pscv_bn_finalize, group after group.
    var = E2 - mean^2 with E2 = ss / n, mean = s / n: one rounding each for the two divisions, three for mean^2 (two inherited from
    mean, one of its own) and one for the difference -> |d var| <= 2^-24 (2 E2 + 3 mean^2) <= 5 2^-24 E2: K = 5 against E[x^2].
    invstd = 1 / sqrt(var + eps): d var / (2 (var + eps)^1.5) (first order, 1 % allowance) + 3 roundings (add, sqrt, divide)."""
    fin, _ = R.bn_finalize(sums, n, bn.weight, bn.bias, eps, momentum)
    G, _, C = fin.shape
    gamma = torch.ones(C, dtype=torch.float64) if bn.weight is None else R.f64(bn.weight)
    beta = torch.zeros(C, dtype=torch.float64) if bn.bias is None else R.f64(bn.bias)
    s = R.f64(sums).reshape(G, 2, C)
    mean, invstd = fin[:, 2], fin[:, 3]
    E2 = s[:, 1] / n
    var = (E2 - mean * mean).clamp(min=0.0)
    d_var = 5 * U32 * E2
    d_mean = U32 * mean.abs()                                            # K = 1: one division
    d_invstd = 1.01 * 0.5 * invstd ** 3 * d_var + 3 * U32 * invstd
    d_scale = gamma.abs() * d_invstd + U32 * fin[:, 0].abs()             # + 1: the product
    d_bias = mean.abs() * d_scale + (d_mean * fin[:, 0].abs()) + 2 * U32 * (beta.abs() + (mean * fin[:, 0]).abs())   # + 2: product, difference
    rm, rv = R.f64(run0[0]).clone(), R.f64(run0[1]).clone()
    d_rm, d_rv = torch.zeros(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
    f = n / max(n - 1, 1)
    for g in range(G):     # running = running (1 - m) + batch m: the batch term's own error, the inherited one, 4 roundings on the terms
        d_rm = d_rm * (1 - momentum) + momentum * d_mean[g] + 4 * U32 * (rm.abs() * (1 - momentum) + mean[g].abs() * momentum)
        d_rv = d_rv * (1 - momentum) + momentum * f * d_var[g] + 5 * U32 * (rv.abs() * (1 - momentum) + var[g] * f * momentum)
        rm = rm * (1 - momentum) + mean[g] * momentum
        rv = rv * (1 - momentum) + var[g] * f * momentum
    return fin, (d_scale, d_bias, d_mean, d_invstd), (rm, rv, d_rm, d_rv), d_var


@pytest.mark.parametrize("C,affine,groups,nvox", [(8, True, 5, 777), (64, True, 1, 777), (128, False, 5, 333), (1024, True, 1, 777),
                                                  (1024, False, 2, 3), (8, True, 1, 1), (64, False, 3, 1)])
def test_bn_finalize(C, affine, groups, nvox):
    """pscv_bn_finalize against float64: C up to the ABI's 1024, gamma / beta absent, a constant channel (variance 0 after the clamp,
    invstd = 1 / sqrt(eps) exactly), one voxel, and groups updating the running statistics in order (num_batches_tracked += groups)."""
    from wild_deep_mvs_amd import ops
    g = R.gen(C, groups, nvox, 5)
    eps, momentum = 2.0 ** -4, 0.25
    y = R.ints(g, (groups, 1, 1, nvox, C), -4, 4, torch.float16)
    y[..., 0] = 3.0                                                       # the constant channel
    sums = R.bn_sums(y, groups).float()                                   # exact: integers below 2^24
    bn = _bn_module(C, affine, eps, momentum, g)
    run0 = (bn.running_mean.clone(), bn.running_var.clone())
    ref, (d_scale, d_bias, d_mean, d_invstd), (rm, rv, d_rm, d_rv), _ = _finalize_bounds(sums, nvox, bn, eps, momentum, run0)
    bn = bn.cuda()
    out = ops.bn_finalize(sums.cuda() if groups > 1 else sums[0].cuda(), nvox, bn)
    out = host(out).reshape(groups, 4, C)
    for k, (name, tol) in enumerate([("scale", d_scale), ("bias", d_bias), ("mean", d_mean), ("invstd", d_invstd)]):
        assert_within(f"bn_finalize {name}", out[:, k], ref[:, k], tol / U32, 1)
    assert_within("running_mean", bn.running_mean, rm, d_rm / U32, 1)
    assert_within("running_var", bn.running_var, rv, d_rv / U32, 1)
    assert int(bn.num_batches_tracked) == groups
    assert bool((out[:, 2, 0] == 3.0).all()) and bool((out[:, 3, 0] == 4.0).all())          # constant channel: mean 3, variance 0 -> 1 / sqrt(2^-4)
    if nvox == 1:
        assert bool((out[:, 3] == 4.0).all())


def test_bn_finalize_variance_cancellation_is_bounded():
    """mean / std = 30: E[x^2] - mean^2 in fp32 loses log2(901) = 10 bits of the variance.  Documented, bounded by
    K 2^-24 E[x^2] with K = 5 (see _finalize_bounds); the measured error is printed (profiles/train_kernels_precision.txt)."""
    from wild_deep_mvs_amd import ops
    C, n = 64, 40037
    g = R.gen(30)
    y = (torch.randn(1, 1, 1, n, C, generator=g) + 30.0).to(torch.float16)
    sums = R.bn_sums(y, 1).float()
    bn = _bn_module(C, True, 1e-5, 0.1, g)
    run0 = (bn.running_mean.clone(), bn.running_var.clone())
    ref, (d_scale, d_bias, d_mean, d_invstd), _, d_var = _finalize_bounds(sums, n, bn, 1e-5, 0.1, run0)
    out = host(ops.bn_finalize(sums[0].cuda(), n, bn.cuda()))
    s = R.f64(sums)[0]
    var_ref = s[1] / n - (s[0] / n) ** 2
    var_got = 1.0 / out[3] ** 2 - 1e-5
    worst = float(((var_got - var_ref).abs() / (U32 * s[1] / n)).max())
    print(f"[precision] bn_finalize variance at mean/std = 30: worst |d var| / (2^-24 E[x^2]) = {worst:.3g} (K = 5), "
          f"relative to the variance itself {float(((var_got - var_ref).abs() / var_ref).max()):.3g}", flush=True)
    assert_within("invstd", out[3], ref[0, 3], d_invstd[0] / U32, 1)
    assert_within("scale", out[0], ref[0, 0], d_scale[0] / U32, 1)


@pytest.mark.parametrize("C,affine,groups", [(8, True, 5), (64, True, 1), (128, False, 2), (1024, True, 1), (1024, False, 3)])
def test_bn_bwd_coeffs(C, affine, groups):
    """pscv_bn_bwd_coeffs: the five rows ca, cb, cc, d gamma, d beta.  With S0 = sum dz, S1 = sum dz y:
    d gamma = invstd (S1 - mean S0): 3 roundings (fused product-difference counted as 2, the scaling) against T2 = invstd (|S1| + |mean S0|);
    ca = gamma invstd: 1;  cb = -ca invstd d gamma / n: 4 of its own + d gamma's 3 -> 7 against (ca invstd / n) T2;
    cc = -ca S0 / n + ca invstd mean d gamma / n: 4 against |ca S0 / n| and 5 + 3 + 1 = 9 against |ca invstd mean / n| T2."""
    from wild_deep_mvs_amd import ops
    g = R.gen(C, groups, 9)
    n = 40037
    sums = torch.randn(groups, 2, C, generator=g) * math.sqrt(n)
    fin = torch.stack([torch.zeros(groups, C), torch.zeros(groups, C), torch.randn(groups, C, generator=g), torch.rand(groups, C, generator=g) + 0.5], 1)
    gamma = (torch.rand(C, generator=g) + 0.5) if affine else None
    finc = fin.cuda()
    if groups == 1:
        got = ops.bn_bwd_coeffs(sums[0].cuda(), finc[0, 2].contiguous(), finc[0, 3].contiguous(), None if gamma is None else gamma.cuda(), n)
    else:
        got = ops.bn_bwd_coeffs(sums.cuda(), finc[:, 2], finc[:, 3], None if gamma is None else gamma.cuda(), n)
    got = host(got).reshape(groups, 5, C)
    ref = R.bn_bwd_coeffs(sums, fin[:, 2], fin[:, 3], gamma, n)
    mean, invstd, S0, S1 = R.f64(fin[:, 2]), R.f64(fin[:, 3]), R.f64(sums[:, 0]), R.f64(sums[:, 1])
    ca = ref[:, 0].abs()
    T2 = invstd * (S1.abs() + (mean * S0).abs())
    assert_within("ca", got[:, 0], ref[:, 0], ca, 1)
    assert_within("cb", got[:, 1], ref[:, 1], ca * invstd / n * T2, 7)
    assert_within("cc", got[:, 2], ref[:, 2], (4 * ca * S0.abs() / n + 9 * ca * invstd * mean.abs() / n * T2), 1)
    assert_within("d gamma", got[:, 3], ref[:, 3], T2, 3)
    assert_bits("d beta", got[:, 4], ref[:, 4])


# =======================================================================================================================
# softmax heads, backward
# =======================================================================================================================
# Measured on the MI355X (profiles/train_kernels_precision.txt): worst (|got - ref| - ulp16 / 2) / (2^-24 T) over all cases below,
# and the bound = 4 x that, rounded up to a power of two.
SOFTARGMIN_K = 2.0 ** 4        # measured 3.04 (all three heads, D = 192, fp16 output)
HEADS = {"depth": (1, 0, 0), "index": (0, 1, 0), "entropy": (0, 0, 1), "all": (1, 1, 1)}


def _softargmin(c, heads, out_dtype, ref_case=None):
    from wild_deep_mvs_amd import ops
    hd, hi, he = HEADS[heads]
    cu = lambda t, on: t.cuda() if on else None
    got = ops.softargmin_bwd(c["logits"].cuda(), cu(c["depth"], hd), cu(c["gd"], hd), out_dtype, grad_index=cu(c["gi"], hi),
                             grad_entropy=cu(c["ge"], he))
    r = ref_case or c
    ref, T = R.softargmin_heads_bwd(r["logits"], r["depth"] if hd else None, r["gd"] if hd else None, r["gi"] if hi else None,
                                    r["ge"] if he else None)
    assert float(got[..., 1:].float().abs().max()) == 0.0, "channels 1-7 must be exactly zero"
    return got[..., 0], ref, T


@pytest.mark.parametrize("out_dtype", R.DT)
@pytest.mark.parametrize("heads", list(HEADS))
@pytest.mark.parametrize("D", R.SOFTARGMIN_D)
def test_softargmin_bwd(D, heads, out_dtype):
    """70 pixels (two blocks of 32 and one of 6: idle lanes clamp to pixel npix - 1) x D from 1 (seven empty depth slices) over 9 and
    33 (ragged slices) to 192; each head alone and all three; a saturated pixel (the 1e-9 clamp of the entropy active) and a pixel
    of all-equal logits are part of every case."""
    got, ref, T = _softargmin(R.softargmin_case(D), heads, out_dtype)
    assert_within(f"softargmin_bwd D={D} {heads}", got, ref, T, SOFTARGMIN_K, out_dtype)


@pytest.mark.parametrize("out_dtype", R.DT)
@pytest.mark.parametrize("D", [9, 33])
def test_softargmin_bwd_per_pixel_planes_and_shifted_logits(D, out_dtype):
    """Depth planes [B,D,h,w]; and the whole volume shifted by +1000.5 (exact in fp32 for these logits): the result stays within
    the same bound of the UNSHIFTED reference -- the maximum is subtracted before anything is exponentiated."""
    got, ref, T = _softargmin(R.softargmin_case(D, per_pixel=True), "all", out_dtype)
    assert_within(f"softargmin_bwd D={D} per-pixel planes", got, ref, T, SOFTARGMIN_K, out_dtype)
    got, ref, T = _softargmin(R.softargmin_case(D, shift=1000.5), "all", out_dtype, ref_case=R.softargmin_case(D))
    assert_within(f"softargmin_bwd D={D} shifted by 1000.5", got, ref, T, SOFTARGMIN_K, out_dtype)


# =======================================================================================================================
# visibility-weighted fusion
# =======================================================================================================================
FUSE_K = 2.0 ** 5          # forward (partial sums, weight sum, normalised volume) and d interm: measured 7.84 (partial sums, 16 views)
FUSE_DU_K = 2.0 ** 5       # d uncert against (w_v / W) sum |G| |I_v - fused|: measured 5.04 (3 views, D = 33)


@pytest.mark.parametrize("dtype", R.DT)
@pytest.mark.parametrize("D", R.FUSE_D)
@pytest.mark.parametrize("n_src", R.FUSE_NSRC)
def test_fuse_pairs_real(n_src, D, dtype):
    """pscv_fuse_pairs (normalised, and partial sums + weight sum), pscv_fuse_finish and pscv_fuse_pairs_bwd with 1 .. PSCV_MAX_SRC
    views, uncertainties over [-8, 8] (weights over seven decades) and depths that leave the backward's eight slices empty (1, 7),
    even (8) or ragged (9, 33)."""
    from wild_deep_mvs_amd import ops
    c = R.fuse_case(n_src, D, dtype)
    I, U, G = [t.cuda() for t in c["I"]], [u.cuda() for u in c["U"]], c["G"].cuda()
    ref, W, T = R.fuse(c["I"], c["U"], True)
    pref, _, pT = R.fuse(c["I"], c["U"], False)
    assert_within("fuse_pairs normalised", ops.fuse_pairs(I, U), ref, T, FUSE_K, dtype)
    part, wsum = ops.fuse_pairs(I, U, normalise=False, want_wsum=True)
    assert_within("fuse_pairs partial sums", part, pref, pT, FUSE_K)
    assert_within("fuse_pairs weight sum", wsum, W, W, FUSE_K)
    out2, wsum2 = ops.fuse_pairs(I, U, want_wsum=True)
    assert torch.equal(out2, ops.fuse_pairs(I, U)) and torch.equal(wsum2, wsum)
    # fuse_finish on the kernel's own fp32 partials: K = 2 roundings (the reciprocal, the product)
    fref = R.fuse_finish(part, wsum)
    assert_within("fuse_finish", ops.fuse_finish(part, wsum, dtype), fref, fref.abs(), 2, dtype)
    dI, dU = ops.fuse_pairs_bwd(I, U, G)
    rI, rU, TU = R.fuse_bwd(c["I"], c["U"], c["G"])
    for v in range(n_src):
        assert_within(f"d interm {v}", dI[v], rI[v], rI[v].abs(), FUSE_K, dtype)
    # d uncert: its terms cancel (sum G I_v against sum G fused), so it is held against the sum of |G| |I_v - fused|, not its own size
    assert_within("d uncert", torch.stack(dU), rU, TU, FUSE_DU_K)
    if n_src == 1:
        assert float(torch.stack(dU).abs().max()) == 0.0      # one view: fused IS that view, the bound is 0


@pytest.mark.parametrize("dtype", R.DT)
@pytest.mark.parametrize("n_src", R.FUSE_NSRC)
def test_fuse_pairs_exact(n_src, dtype):
    """Integer volumes and uncertainty 0 (weight exactly 1): partial sums and the weight sum are exact for any view count, the
    normalised volume and both gradients for power-of-two counts."""
    from wild_deep_mvs_amd import ops
    c = R.fuse_case(n_src, 9, dtype, exact=True)
    I, U, G = [t.cuda() for t in c["I"]], [u.cuda() for u in c["U"]], c["G"].cuda()
    part, wsum = ops.fuse_pairs(I, U, normalise=False, want_wsum=True)
    pref, W, _ = R.fuse(c["I"], c["U"], False)
    assert_bits("partial sums", part, pref)
    assert_bits("weight sum", wsum, W)
    if n_src != 3:
        ref = R.fuse(c["I"], c["U"], True)[0]
        assert_bits("normalised", ops.fuse_pairs(I, U), ref)
        assert_bits("fuse_finish", ops.fuse_finish(part, wsum, dtype), ref)
        dI, dU = ops.fuse_pairs_bwd(I, U, G)
        rI, rU, _ = R.fuse_bwd(c["I"], c["U"], c["G"])
        assert_bits("d interm", torch.stack(dI), rI)
        assert_bits("d uncert", torch.stack(dU), rU)


# =======================================================================================================================
# weight gradient
# =======================================================================================================================
def _wgrad_plan(ca, cb, stride, grid):
    """(workgroups along x, tiles, k-steps per tile) of the launch ops.conv3d_wgrad makes."""
    from wild_deep_mvs_amd import _lib as L
    ca16, cb16 = (ca + 15) // 16 * 16, (cb + 15) // 16 * 16
    nblk = L.lib().pscv_conv3d_wgrad_workspace(*grid, ca, cb, stride) // (27 * ca16 * cb16)
    tiles, ksteps = R.wgrad_tiles(grid, stride)
    return nblk, tiles, ksteps


@pytest.mark.parametrize("dtype", R.DT)
@pytest.mark.parametrize("ca,cb,stride,grid,tag", R.WGRAD_CASES)
def test_conv3d_wgrad_exact(ca, cb, stride, grid, tag, dtype):
    """Integers in [-2, 2]: pscv_conv3d_wgrad equals the 27 float64 matrix products bit for bit -- for grids smaller than a tile,
    with odd depth (half-empty two-plane tiles), ragged rows and width 16 + 1, exactly one tile, half-empty channel tiles (24, 40, 56)
    and, per kernel instance, a grid with more tiles than workgroups, whose accumulators stay in registers from tile to tile."""
    from wild_deep_mvs_amd import ops
    nblk, tiles, _ = _wgrad_plan(ca, cb, stride, grid)
    assert (nblk < tiles) if tag == "multi-tile" else (nblk == tiles), (nblk, tiles)
    P, Q, coff = R.wgrad_case(ca, cb, stride, grid, dtype, True)
    dw = ops.conv3d_wgrad(P.cuda(), Q.cuda(), ca=ca, cb=cb, stride=stride)
    assert_bits(f"wgrad {ca}x{cb} s{stride} {grid}", dw, R.wgrad_ref(P, Q, coff, ca, cb, stride))


WG_REAL = [c for c in R.WGRAD_CASES if c[4] == "small"] + [c for c in R.WGRAD_CASES if c[4] == "multi-tile" and c[0] * c[1] <= 64 * 32 and c[3][1] > 1]


@pytest.mark.parametrize("dtype", R.DT)
@pytest.mark.parametrize("ca,cb,stride,grid,tag", WG_REAL)
def test_conv3d_wgrad_real(ca, cb, stride, grid, tag, dtype):
    """|dw - ref| <= K 2^-24 wgrad(|P|, |Q|).  One output passes through: per tile of its workgroup `ksteps` MFMAs of 32 products each
    (exact products, at most 32 additions per MFMA), over ceil(tiles / nblk) tiles; then the finishing kernel: ceil(nblk / 32) rows in each
    of two accumulators, 1 to join them, 16 slices.  The relative-L2 bound of tests/test_gpu_train.py is kept."""
    from wild_deep_mvs_amd import ops
    from _util import check_close
    nblk, tiles, ksteps = _wgrad_plan(ca, cb, stride, grid)
    K = -(-tiles // nblk) * ksteps * 32 + (-(-nblk // 32) + 1 + 16)
    P, Q, coff = R.wgrad_case(ca, cb, stride, grid, dtype, False)
    dw = ops.conv3d_wgrad(P.cuda(), Q.cuda(), ca=ca, cb=cb, stride=stride)
    ref = R.wgrad_ref(P, Q, coff, ca, cb, stride)
    assert_within(f"wgrad {ca}x{cb} s{stride} {grid}", dw, ref, R.wgrad_ref(P, Q, coff, ca, cb, stride, absolute=True), K)
    check_close("dW", dw.cpu(), ref.float(), rel_l2=2e-5)


@pytest.mark.parametrize("dtype", R.DT)
@pytest.mark.parametrize("ca,cb,stride,grid", [(24, 40, 1, (2, 3, 7, 17)), (64, 32, 2, (2, 3, 7, 17)), (8, 8, 1, (2, 3, 7, 17)),
                                               (40, 24, 1, (1, 1, 9, 21)), (64, 64, 1, (2, 1, 11, 37))])
def test_conv3d_wgrad_channel_slices(ca, cb, stride, grid, dtype):
    """P and Q as the 8-aligned channel slices [8 : 8 + c] of tensors 16 channels wider (p_coff = q_coff = 8), 3-D and single-plane:
    the bits of the dense call, and nothing of the neighbouring channels."""
    from wild_deep_mvs_amd import ops
    P, Q, coff = R.wgrad_case(ca, cb, stride, grid, dtype, True, wider=16)
    assert coff == 8 and P.shape[4] >= ca + 16 and Q.shape[4] >= cb + 16
    dw = ops.conv3d_wgrad(P.cuda(), Q.cuda(), ca=ca, cb=cb, stride=stride, p_coff=coff, q_coff=coff)
    assert_bits("wgrad on channel slices", dw, R.wgrad_ref(P, Q, coff, ca, cb, stride))


@pytest.mark.parametrize("dtype", R.DT)
@pytest.mark.parametrize("ca,cb,stride,grid", [(16, 8, 2, (2, 3, 7, 17)), (24, 40, 1, (2, 3, 7, 17)), (8, 8, 1, (2, 1, 11, 37)), (64, 32, 1, (1, 1, 9, 21))])
def test_conv3d_wgrad_accumulate(ca, cb, stride, grid, dtype):
    """accumulate = 1 through the C ABI (ops.conv3d_wgrad passes 0): dw = prefill + gradient; in single-plane mode the taps of the
    kernel slices tz != 1, which that mode never computes, keep their prefill bit for bit."""
    from wild_deep_mvs_amd import _lib as L, ops
    P, Q, coff = R.wgrad_case(ca, cb, stride, grid, dtype, True)
    g = R.gen(ca, cb, 3)
    pre = torch.randint(-100, 101, (ca, cb, 3, 3, 3), generator=g).float()
    plane = grid[1] == 1 and stride == 1
    if plane:       # tz = 0 and 2 only ever meet the zero padding: any bit pattern must survive
        pre[:, :, 0] = torch.randn(ca, cb, 3, 3, generator=g)
        pre[:, :, 2] = -torch.randn(ca, cb, 3, 3, generator=g) * 1e-3
    p, q, dw = P.cuda(), Q.cuda(), pre.cuda()
    ws = ops._workspace(p.device, L.lib().pscv_conv3d_wgrad_workspace(*grid, ca, cb, stride))
    rc = L.lib().pscv_conv3d_wgrad(ops._p(p), p.shape[4], coff, ca, ops._p(q), q.shape[4], coff, cb, ops._dt(p), *grid, stride, ops._p(ws), ops._p(dw), 1, ops._stream())
    L.check(rc, "pscv_conv3d_wgrad")
    assert_bits("prefill + gradient", dw, pre.double() + R.wgrad_ref(P, Q, coff, ca, cb, stride))
    if plane:
        assert torch.equal(dw.cpu()[:, :, [0, 2]].view(torch.int32), pre[:, :, [0, 2]].view(torch.int32))


# =======================================================================================================================
# NaN and saturation through 16-bit stores
# =======================================================================================================================
def assert_nan_like(name, got, ref, dtype):
    """NaN at exactly the elements where the float64 reference is NaN (not +-65504, not 0); everything else the reference's bits."""
    got, ref = host(got), R.round16(ref, dtype).reshape(got.shape)
    gn, rn = torch.isnan(got), torch.isnan(ref)
    assert int(rn.sum()) > 0, f"{name}: the case holds no NaN"
    if not torch.equal(gn, rn):
        i = tuple(torch.nonzero(gn != rn)[0].tolist())
        raise AssertionError(f"{name}: NaN at {int(gn.sum())} elements, reference at {int(rn.sum())}; first difference at {i}: got {float(got[i])!r}, "
                             f"ref {float(ref[i])!r}")
    assert torch.equal(got[~rn], ref[~rn]), name


def _poison(t, g, k=5):
    t = t.clone()
    idx = torch.randint(0, t.numel(), (k,), generator=g)
    t.view(-1)[idx] = float("nan")
    return t


@pytest.mark.parametrize("dtype", R.DT)
def test_nan_survives_the_16_bit_stores_of_the_training_kernels(dtype):
    """A NaN activation or gradient must stay NaN through bn_act, bn_bwd_apply, relu_bwd and relu_bwd_sum (and reach the channel
    sum) in both storage types.  (The fp16 pack once clamped to +-65504 with v_med3, which returns a non-NaN operand: -65504.)"""
    from wild_deep_mvs_amd import ops
    C, nvox = 16, 777
    c = R.bn_case(C, nvox, 1, dtype, True)
    g = R.gen(99)
    c["y"], c["dact"], c["skip"] = _poison(c["y"], g), _poison(c["dact"], g), _poison(c["skip"], g)
    d = bn_gpu(c, 1)
    sc, bi, ca, cb, cc = cpu_rows(c)
    for relu, skip in ACT_VARIANTS:
        got = ops.bn_act(d["y"], d["scale"], d["bias"], relu=relu, skip=d["skip"] if skip else None)
        assert_nan_like(f"bn_act relu={relu} skip={skip}", got, R.bn_act(c["y"], sc, bi, relu, c["skip"] if skip else None)[0], dtype)
    for relu in (False, True):
        got = ops.bn_bwd_apply(d["dact"], d["y"], d["scale"], d["bias"], d["ca"], d["cb"], d["cc"], relu=relu)
        assert_nan_like(f"bn_bwd_apply relu={relu}", got, R.bn_bwd_apply(c["dact"], c["y"], sc, bi, ca, cb, cc, relu)[0], dtype)
    for slope in (0.0, 0.5):
        rd, _, rsum = R.relu_bwd(c["dact"], c["y"], slope, dtype)
        assert_nan_like(f"relu_bwd slope={slope}", ops.relu_bwd(d["dact"], d["y"], slope), rd, dtype)
        dpre, ssum = ops.relu_bwd_sum(d["dact"], d["y"], slope)
        assert_nan_like(f"relu_bwd_sum slope={slope}: dpre", dpre, rd, dtype)
        ssum = host(ssum)
        assert torch.equal(torch.isnan(ssum), torch.isnan(rsum)) and torch.equal(ssum[~torch.isnan(rsum)], rsum[~torch.isnan(rsum)])
        assert 0 < int(torch.isnan(rsum).sum()) < C


@pytest.mark.parametrize("dtype", R.DT)
def test_nan_survives_the_16_bit_stores_of_the_fusion(dtype):
    from wild_deep_mvs_amd import ops
    c = R.fuse_case(2, 9, dtype, exact=True)
    g = R.gen(98)
    c["I"][1] = _poison(c["I"][1], g)
    I, U = [t.cuda() for t in c["I"]], [u.cuda() for u in c["U"]]
    ref = R.fuse(c["I"], c["U"], True)[0]
    assert_nan_like("fuse_pairs", ops.fuse_pairs(I, U), ref, dtype)
    part, wsum = ops.fuse_pairs(I, U, normalise=False, want_wsum=True)
    assert_nan_like("fuse_finish", ops.fuse_finish(part, wsum, dtype), ref, dtype)


def test_fp16_stores_saturate_at_65504():
    """include/pscv.h: a finite result beyond the fp16 range is stored as +-65504, never as inf."""
    from wild_deep_mvs_amd import ops
    dtype = torch.float16
    C, nvox = 8, 777
    c = R.bn_case(C, nvox, 1, dtype, True)
    c["fin"][:, 0] *= 2.0 ** 14                       # |y * scale| up to 2^17
    c["co"][:, 0] *= 2.0 ** 14
    d = bn_gpu(c, 1)
    sc, bi, ca, cb, cc = cpu_rows(c)
    for relu in (False, True):
        ref = R.bn_act(c["y"], sc, bi, relu, c["skip"])[0]
        assert float(ref.abs().max()) > 65504
        assert_bits(f"bn_act relu={relu}", ops.bn_act(d["y"], d["scale"], d["bias"], relu=relu, skip=d["skip"]), ref, dtype)
        ref = R.bn_bwd_apply(c["dact"], c["y"], sc, bi, ca, cb, cc, relu)[0]
        assert float(ref.max()) > 65504 and float(ref.min()) < -65504
        assert_bits(f"bn_bwd_apply relu={relu}", ops.bn_bwd_apply(d["dact"], d["y"], d["scale"], d["bias"], d["ca"], d["cb"], d["cc"], relu=relu), ref, dtype)
    f = R.fuse_case(2, 9, dtype, exact=True)
    part = (R.fuse(f["I"], f["U"], False)[0] * 2.0 ** 15).float()
    wsum = torch.full((2, 5, 7), 2.0)
    ref = R.fuse_finish(part, wsum)
    assert float(ref.max()) > 65504 and float(ref.min()) < -65504
    assert_bits("fuse_finish", ops.fuse_finish(part.cuda(), wsum.cuda(), dtype), ref, dtype)


@pytest.mark.parametrize("cin,cout,kind,shape", [(32, 8, 0, (16, 16, 32)), (16, 16, 0, (6, 10, 21)), (8, 16, 1, (16, 16, 32)), (16, 8, 2, (4, 8, 16))])
@pytest.mark.parametrize("relu", [True, False])
def test_conv3d_epilogue_keeps_nan_in_an_fp16_output(cin, cout, kind, shape, relu):
    """tests/test_gpu_conv3d.py::test_conv3d_epilogue_propagates_nan_like_torch_relu asks for an fp32 output; here the epilogue stores
    fp16 (out_dtype=None): every voxel ATen poisons is NaN, none became +-65504 or 0."""
    import numpy as np
    from wild_deep_mvs_amd import _lib as L, ops
    g = torch.Generator().manual_seed(3)
    D, H, W = shape
    transposed = kind == L.CONV_T2
    x = torch.randn(1, cin, D, H, W, generator=g).to(torch.bfloat16).float()
    x[0, 1, D // 2, H // 2, W // 2] = float("nan")
    w = (torch.randn((cin, cout, 3, 3, 3) if transposed else (cout, cin, 3, 3, 3), generator=g) / np.sqrt(27 * cin)).to(torch.bfloat16).float()
    layer = ops.Conv3dLayer.build(w, kind=kind, transposed=transposed, device="cuda", relu=relu, dtype=torch.float16)
    y = ops.conv3d(ops.to_channels_last(x.cuda(), torch.float16), layer)
    assert y.dtype == torch.float16
    ref = F.conv_transpose3d(x, w, stride=2, padding=1, output_padding=1) if transposed else F.conv3d(x, w, stride=1 if kind == L.CONV_S1 else 2, padding=1)
    ref = F.relu(ref) if relu else ref
    got = y.permute(0, 4, 1, 2, 3).float().cpu()
    gn, rn = torch.isnan(got), torch.isnan(ref)
    assert int(rn.sum()) > 0 and bool((gn | ~rn).all()), (int(gn.sum()), int(rn.sum()), got[rn & ~gn][:8].tolist())
    assert not torch.isinf(got).any()
