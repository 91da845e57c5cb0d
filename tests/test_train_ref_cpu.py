"""tests/_train_ref.py against itself and against float64 autograd of the torch modules (no GPU), and the conditions that
tests/test_gpu_train_kernels.py relies on, checked on the very inputs the GPU tests build:
  * every integer-valued case keeps all partial sums below 2^24 (any fp32 summation order then gives the same bits) and every
    stored result exactly representable in the storage type;
  * no ReLU sign test of a real-valued case lies within fp32 rounding of zero;
  * every weight-gradient shape tagged "multi-tile" has more tiles than the plan launches workgroups."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import _train_ref as R

F64 = torch.float64
CL = lambda x: x.permute(0, 2, 3, 4, 1).contiguous()      # NCDHW -> channels-last
CF = lambda x: x.permute(0, 4, 1, 2, 3)                   # and back (view)


def close(got, ref, tol=1e-11):
    scale = float(ref.abs().max()) + 1e-300
    err = float((got - ref).abs().max())
    assert err <= tol * scale, (err, scale)


# ---- round16 / ulp16 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", R.DT)
def test_round16_is_torch_rounding_with_saturation_and_nan(dtype):
    g = torch.Generator().manual_seed(1)
    x = torch.randn(200000, generator=g) * torch.exp(torch.randn(200000, generator=g) * 6)     # fp32 values over many binades
    x = torch.cat([x, torch.tensor([0.0, -0.0, 65504.0, 65519.9, -65519.9, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 6e-8, 1e-40])])
    ref = x.to(dtype).double()
    if dtype == torch.float16:
        ref = ref.clamp(-65504.0, 65504.0)
    assert torch.equal(R.round16(x.double(), dtype), ref)
    sp = torch.tensor([float("nan"), float("inf"), -float("inf"), 1e6, -1e6, 65520.0], dtype=F64)
    r = R.round16(sp, dtype)
    assert torch.isnan(r[0])
    if dtype == torch.float16:
        assert r[1:].tolist() == [65504.0, -65504.0, 65504.0, -65504.0, 65504.0]
    else:
        assert r[1:].tolist() == [float("inf"), -float("inf"), 999424.0, -999424.0, 65536.0]
    # one rounding: 1 + 2^-11 + 2^-30 is above the fp16 tie; through fp32 it would first fall ON the tie and then round to even (1.0)
    v = torch.tensor([1.0 + 2.0 ** -11 + 2.0 ** -30, 1.0 + 2.0 ** -8 + 2.0 ** -30], dtype=F64)
    up = R.round16(v, dtype)
    assert float(up[0 if dtype == torch.float16 else 1]) == 1.0 + (2.0 ** -10 if dtype == torch.float16 else 2.0 ** -7)
    # ulp16: the spacing torch's own grid has
    y = x[:1000].to(dtype)
    nxt = torch.nextafter(y, torch.full_like(y, float("inf"))) if dtype == torch.float16 else None
    if nxt is not None:
        fin = torch.isfinite(nxt) & (y >= 0)
        assert torch.equal(R.ulp16(y.double(), dtype)[fin], (nxt.double() - y.double())[fin])
    assert float(R.ulp16(torch.tensor([1.0]), dtype)) == 2.0 ** -R.MANT[dtype]
    assert float(R.ulp16(torch.tensor([0.0]), dtype)) == 2.0 ** (R.EMIN[dtype] - R.MANT[dtype])


# ---- BatchNorm in train() against the module --------------------------------------------------------------------------------
@pytest.mark.parametrize("relu", [False, True, "post"])
@pytest.mark.parametrize("affine", [True, False])
def test_bn_chain_equals_batchnorm3d_autograd(relu, affine):
    g = torch.Generator().manual_seed(5)
    C, shape = 8, (2, 8, 2, 3, 5)
    y = (torch.randn(shape, generator=g, dtype=F64) * 1.5 + 0.3).requires_grad_(True)
    skip = torch.randn(shape, generator=g, dtype=F64)
    dact = torch.randn(shape, generator=g, dtype=F64)
    bn = nn.BatchNorm3d(C, affine=affine, momentum=0.3).double().train()
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(C, generator=g, dtype=F64)); bn.running_var.copy_(torch.rand(C, generator=g, dtype=F64) + 0.5)
        if affine:
            bn.weight.copy_(torch.rand(C, generator=g, dtype=F64) + 0.5); bn.bias.copy_(torch.randn(C, generator=g, dtype=F64))
    run0 = (bn.running_mean.clone(), bn.running_var.clone())
    z = bn(y)
    out = F.relu(z) + skip if relu is True else (F.relu(z + skip) if relu == "post" else z + skip)
    out.backward(dact)
    n = y.numel() // C
    ycl = CL(y.detach())
    sums = R.bn_sums(ycl)
    fin, (rm, rv) = R.bn_finalize(sums, n, bn.weight, bn.bias, bn.eps, bn.momentum, run0)
    close(rm, bn.running_mean); close(rv, bn.running_var)
    scale, bias, mean, invstd = fin[0]
    got, T = R.bn_act(ycl, scale, bias, relu, CL(skip))
    close(CF(got), out.detach())
    assert bool((T >= got.abs() * (1 - 1e-12)).all())
    dpre = CL(dact)
    if relu == "post":
        dpre = R.relu_bwd(dpre, CL(out.detach()), 0.0, torch.float16)[0]
    bs = R.bn_bwd_sums(dpre, ycl, scale, bias, relu is True)
    co = R.bn_bwd_coeffs(bs, mean, invstd, bn.weight, n)[0]
    dy, Td = R.bn_bwd_apply(dpre, ycl, scale, bias, co[0], co[1], co[2], relu is True)
    close(CF(dy), y.grad, 1e-10)
    if affine:
        close(co[3], bn.weight.grad, 1e-10); close(co[4], bn.bias.grad, 1e-10)


def test_bn_finalize_groups_update_the_running_statistics_in_order():
    g = torch.Generator().manual_seed(6)
    C, G = 16, 5
    y = torch.randn(G, C, 1, 4, 6, generator=g, dtype=F64) * torch.arange(1, G + 1, dtype=F64).view(G, 1, 1, 1, 1)
    bn = nn.BatchNorm3d(C).double().train()
    outs = [bn(y[i:i + 1]) for i in range(G)]
    n = 24
    fin, (rm, rv) = R.bn_finalize(R.bn_sums(CL(y), G), n, bn.weight, bn.bias, bn.eps, bn.momentum, (torch.zeros(C), torch.ones(C)))
    close(rm, bn.running_mean); close(rv, bn.running_var)
    for i in range(G):
        got, _ = R.bn_act(CL(y[i:i + 1]), fin[i, 0], fin[i, 1], False)
        close(CF(got), outs[i].detach())
    allg, _ = R.bn_act(CL(y), fin[:, 0], fin[:, 1], False)          # the grouped call is the per-group calls
    close(CF(allg), torch.cat(outs).detach())
    # nvox = 1: the unbiased factor is n / max(n - 1, 1) = 1 and the variance is 0
    fin1, (rm1, rv1) = R.bn_finalize(torch.tensor([[[3.0], [9.0]]]), 1, None, None, 0.25, 0.5, (torch.zeros(1), torch.ones(1)))
    assert fin1[0, :, 0].tolist() == [2.0, -6.0, 3.0, 2.0] and float(rm1) == 1.5 and float(rv1) == 0.5
    # a variance that cancels below zero is clamped
    fin2, _ = R.bn_finalize(torch.tensor([[[3.0], [2.9999]]]), 3, None, None, 0.25, 0.5)
    assert float(fin2[0, 3, 0]) == 2.0


def test_leaky_relu_backward_from_the_output_equals_autograd():
    g = torch.Generator().manual_seed(7)
    x = torch.randn(2, 8, 2, 3, 5, generator=g, dtype=F64).requires_grad_(True)
    out = F.leaky_relu(x, 0.1)
    dout = torch.randn(x.shape, generator=g, dtype=F64)
    out.backward(dout)
    dpre, stored, sums = R.relu_bwd(CL(dout), CL(out.detach()), 0.1, torch.bfloat16)
    close(CF(dpre), x.grad, 1e-7)                      # (slope is the fp32 0.1 the ABI receives)
    assert torch.equal(stored, R.round16(dpre, torch.bfloat16)) and torch.equal(sums, stored.reshape(-1, 8).sum(0))


# ---- softmax heads -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heads", ["depth", "index", "entropy", "all"])
@pytest.mark.parametrize("per_pixel", [False, True])
def test_softargmin_heads_equal_autograd(heads, per_pixel):
    c = R.softargmin_case(9, per_pixel=per_pixel)
    l = c["logits"].double().requires_grad_(True)
    B, D, h, w = l.shape
    p = F.softmax(l, 1)
    dep = c["depth"].double()
    dv = dep if per_pixel else dep.view(B, D, 1, 1)
    loss = 0.0
    kw = {}
    if heads in ("depth", "all"):
        loss = loss + ((p * dv).sum(1) * c["gd"].double()).sum(); kw.update(depth=c["depth"], g_depth=c["gd"])
    if heads in ("index", "all"):
        loss = loss + ((p * torch.arange(D, dtype=F64).view(1, D, 1, 1)).sum(1) * c["gi"].double()).sum(); kw.update(g_index=c["gi"])
    if heads in ("entropy", "all"):
        loss = loss + ((-p * p.clamp(1e-9, 1.0).log()).sum(1) * c["ge"].double()).sum(); kw.update(g_entropy=c["ge"])
    loss.backward()
    got, T = R.softargmin_heads_bwd(c["logits"], **kw)
    close(got, l.grad, 1e-10)
    assert bool((T >= got.abs() * (1 - 1e-12)).all())
    if heads in ("entropy", "all"):
        assert int((p[0, :, 0, 0] <= 1e-9).sum()) == D - 1     # the saturated pixel has the clamp active everywhere but at its peak


def test_softargmin_reference_is_shift_invariant_and_the_shift_is_exact_in_fp32():
    a, b = R.softargmin_case(24), R.softargmin_case(24, shift=1000.5)
    assert torch.equal((b["logits"].double() - 1000.5), a["logits"].double())
    ga, _ = R.softargmin_heads_bwd(a["logits"], a["depth"], a["gd"], a["gi"], a["ge"])
    gb, _ = R.softargmin_heads_bwd(b["logits"], b["depth"], b["gd"], b["gi"], b["ge"])
    close(gb, ga, 1e-12)


# ---- fusion ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_src", [1, 3])
def test_fusion_equals_autograd(n_src):
    c = R.fuse_case(n_src, 7, torch.float16)
    I = [t.double().requires_grad_(True) for t in c["I"]]
    U = [u.double().requires_grad_(True) for u in c["U"]]
    ws = [(-u).exp()[:, None, :, :, None] for u in U]
    fused = sum(i * w for i, w in zip(I, ws)) / sum(ws)
    fused.backward(c["G"].double())
    out, W, T = R.fuse(c["I"], c["U"], True)
    close(out, fused.detach())
    part, W2, _ = R.fuse(c["I"], c["U"], False)
    close(R.fuse_finish(part, W2), fused.detach())
    dI, dU, TU = R.fuse_bwd(c["I"], c["U"], c["G"])
    for v in range(n_src):
        close(dI[v], I[v].grad, 1e-10)
        # (autograd differentiates sum w I / W as written: its own d uncert cancels to rounding noise of sum |G I|, also for one view)
        assert float((dU[v] - U[v].grad).abs().max()) <= 1e-12 * float((c["G"].double().abs() * c["I"][v].double().abs()).sum((1, 4)).max())
    if n_src == 1:
        assert float(dU.abs().max()) == 0.0 and float(TU.abs().max()) == 0.0


# ---- weight gradient ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("grid", [(2, 3, 4, 5), (1, 1, 3, 4)])
def test_wgrad_equals_conv_autograd(stride, transposed, grid):
    g = torch.Generator().manual_seed(8)
    B, D, H, W = grid
    ca, cb = 3, 2
    w = torch.randn(ca, cb, 3, 3, 3, generator=g, dtype=F64).requires_grad_(True)
    if not transposed:     # Conv3d weight [Co = ca, Ci = cb]: P = grad of the output, Q = the input
        x = torch.randn(B, cb, stride * D, stride * H, stride * W, generator=g, dtype=F64)
        y = F.conv3d(x, w, None, stride=stride, padding=1)
        dy = torch.randn(y.shape, generator=g, dtype=F64)
        y.backward(dy)
        P, Q = CL(dy), CL(x)
    else:                  # ConvTranspose3d weight [Ci = ca, Co = cb]: P = the input, Q = grad of the output
        x = torch.randn(B, ca, D, H, W, generator=g, dtype=F64)
        y = F.conv_transpose3d(x, w, None, stride=stride, padding=1, output_padding=stride - 1)
        dy = torch.randn(y.shape, generator=g, dtype=F64)
        y.backward(dy)
        P, Q = CL(x), CL(dy)
    close(R.wgrad(P, Q, stride), w.grad, 1e-12)
    assert bool((R.wgrad(P, Q, stride, absolute=True) >= R.wgrad(P, Q, stride).abs() * (1 - 1e-12)).all())


# ---- the conditions the GPU tests rely on ---------------------------------------------------------------------------------------------
LIM = 2.0 ** 24
EXACT_BN = R.BN_SMALL + [R.RED_MULTI] + R.RED_GROUPED + R.ELEM_GROUPED


@pytest.mark.parametrize("dtype", R.DT)
@pytest.mark.parametrize("C,nvox,groups", EXACT_BN)
def test_exact_bn_cases_are_exact(C, nvox, groups, dtype):
    c = R.bn_case(C, nvox, groups, dtype, True)
    sc, bi = c["fin"][:, 0], c["fin"][:, 1]
    assert float(R.bn_sums(c["y"], groups, absolute=True).max()) < LIM
    assert float(R.bn_bwd_sums(c["dact"], c["y"], sc, bi, False, absolute=True).max()) < LIM
    assert float(c["dact"].double().abs().reshape(-1, C).sum(0).max()) < LIM            # relu_bwd_sum (slope <= 1)
    assert int(R.relu_near_zero(c["y"], sc, bi).sum()) == 0 and float((R.f64(c["y"]).reshape(groups, -1, C) * R.f64(sc)[:, None] + R.f64(bi)[:, None]).abs().min()) >= 0.5
    if c["y"].numel() > 1 << 20:        # (the large reduction shapes feed the reductions only)
        return
    for relu in (False, True, "post"):
        for skip in (None, c["skip"]):
            o, _ = R.bn_act(c["y"], sc, bi, relu, skip)
            assert torch.equal(R.round16(o, dtype), o) and torch.equal(o.float().double(), o)
    for relu in (False, True):
        o, _ = R.bn_bwd_apply(c["dact"], c["y"], sc, bi, c["co"][:, 0], c["co"][:, 1], c["co"][:, 2], relu)
        assert torch.equal(R.round16(o, dtype), o)
    for slope in (0.0, 0.5):
        dpre, stored, _ = R.relu_bwd(c["dact"], c["y"], slope, dtype)
        assert torch.equal(stored, dpre)


@pytest.mark.parametrize("dtype", R.DT)
def test_exact_multi_pass_case_is_exact(dtype):
    C, nvox, groups = R.ELEM_MULTI
    c = R.bn_case(C, nvox, groups, dtype, True)
    o, _ = R.bn_act(c["y"], c["fin"][:, 0], c["fin"][:, 1], "post", c["skip"])
    assert torch.equal(R.round16(o, dtype), o)
    assert nvox * (C // 8) > 8192 * 256 and (nvox * (C // 8)) % 256 != 0


@pytest.mark.parametrize("dtype", R.DT)
@pytest.mark.parametrize("C,nvox,groups", R.BN_SMALL + R.ELEM_GROUPED + [R.RED_MULTI])
def test_real_bn_cases_have_no_sign_test_within_rounding_of_zero(C, nvox, groups, dtype):
    c = R.bn_case(C, nvox, groups, dtype, False)
    assert int(R.relu_near_zero(c["y"], c["fin"][:, 0], c["fin"][:, 1]).sum()) == 0


def test_reduction_shapes_take_the_steps_they_are_meant_to():
    for C, nvox, groups in R.BN_SMALL:
        assert (nvox * (C // 8)) % 256 != 0
    C, nvox, groups = R.RED_MULTI
    assert nvox * (C // 8) > 1024 * 256 and R.red_geometry(nvox * (C // 8), 1) == (1024, 2)
    for C, nvox, groups in R.RED_GROUPED:
        nb, steps = R.red_geometry(nvox * (C // 8), groups)
        assert nb == 1024 // groups and steps >= 2 and (nvox * (C // 8)) % 256 != 0
    assert [g for _, _, g in R.RED_GROUPED] == [2, 5, 256]


def test_fusion_exact_case_is_exact():
    for n in R.FUSE_NSRC:
        c = R.fuse_case(n, 9, torch.bfloat16, exact=True)
        part, W, _ = R.fuse(c["I"], c["U"], False)
        assert torch.equal(W, torch.full_like(W, float(n))) and torch.equal(part.float().double(), part)
        if n in (1, 2, 16):
            o, _, _ = R.fuse(c["I"], c["U"], True)
            assert torch.equal(R.round16(o, torch.bfloat16), o) and torch.equal(R.round16(o, torch.float16), o)


@pytest.mark.parametrize("ca,cb,stride,grid,tag", R.WGRAD_CASES)
def test_wgrad_cases_are_exact_and_multi_tile_where_tagged(ca, cb, stride, grid, tag):
    from wild_deep_mvs_amd import _lib as L
    P, Q, coff = R.wgrad_case(ca, cb, stride, grid, torch.bfloat16, True)
    assert float(R.wgrad_ref(P, Q, coff, ca, cb, stride, absolute=True).max()) < LIM
    assert 4 * grid[0] * grid[1] * grid[2] * grid[3] < LIM          # (any seed and either storage type: |P Q| <= 4 per voxel)
    tiles, _ = R.wgrad_tiles(grid, stride)
    ca16, cb16 = (ca + 15) // 16 * 16, (cb + 15) // 16 * 16
    nblk = L.lib().pscv_conv3d_wgrad_workspace(*grid, ca, cb, stride) // (27 * ca16 * cb16)
    assert nblk >= 1
    if tag == "multi-tile":
        assert nblk < tiles, (nblk, tiles)
    else:
        assert nblk == tiles


def test_wgrad_cases_reach_all_eight_kernel_instances():
    seen = set()
    for ca, cb, stride, grid, tag in R.WGRAD_CASES:
        if tag != "multi-tile":
            continue
        plane = grid[1] == 1 and stride == 1
        seen.add((stride, plane, ((cb + 15) // 16) % 2 == 0, plane and ((ca + 15) // 16) % 4 == 0))
    assert len(seen) == 8, sorted(seen)
