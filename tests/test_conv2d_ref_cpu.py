"""No GPU: the float64 reference of tests/_conv2d_ref.py pinned to ATen, the parity decompositions it is used with, the host weight
packer contracted the way conv2d_kernel contracts it, the argument checks of pscv_conv2d_ex, and the case table that
tests/test_gpu_conv2d_ref.py runs checked against the dispatch table of csrc/conv2d.hip and for the conditions its bounds need."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _conv2d_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


def _engine():
    """(_lib, ops) with libpscv.so loaded; the tests that need the host library skip where it is not built."""
    from wild_deep_mvs_amd import _lib as L, ops
    if not os.path.exists(L.LIB_PATH):
        pytest.skip("libpscv.so is not built")
    L.lib()
    return L, ops


def _nchw(y):
    return y.permute(0, 3, 1, 2)


def _aten(x, w, k, stride):
    """float64 F.conv2d of channels-last x; k2: taps (i + ty, j + tx), one zero row / column past the input."""
    xn = _nchw(x.double())[:, :w.shape[1]]
    if k == 2:
        return F.conv2d(F.pad(xn, (0, 1, 0, 1)), w.double()).permute(0, 2, 3, 1)
    return F.conv2d(xn, w.double(), stride=stride, padding=k // 2).permute(0, 2, 3, 1)


@pytest.mark.parametrize("k,stride", [(3, 1), (3, 2), (5, 2), (1, 1), (1, 2), (2, 1)])
def test_reference_equals_float64_aten(k, stride):
    g = torch.Generator().manual_seed(10 * k + stride)
    for B, Hi, Wi, ci, cpad, co in [(2, 1, 1, 3, 8, 4), (1, 2, 2, 8, 8, 20), (2, 2, 1, 5, 8, 8), (3, 7, 10, 16, 16, 12), (1, 9, 13, 8, 8, 16), (2, 6, 5, 3, 8, 8)]:
        x = torch.randn(B, Hi, Wi, cpad, generator=g).to(torch.float16)         # (channels past c_in hold values: they must not be read)
        w = torch.randn(co, ci, k, k, generator=g).to(torch.float16).float()
        r = R.conv2d(x, w, k=k, stride=stride)
        want = _aten(x, w, k, stride)
        assert r.y.shape == want.shape == (B,) + R.out_hw(Hi, Wi, k, stride) + (co,)
        torch.testing.assert_close(r.y, want, rtol=0, atol=1e-12 * float(want.abs().max()))
        torch.testing.assert_close(r.U, _aten(x.abs(), w.abs(), k, stride), rtol=0, atol=1e-12 * float(r.U.max()))
        assert r.K == 32 * -(-k * k * cpad // 32) and torch.equal(r.y, r.v)
    with pytest.raises(ValueError):
        R.geometry(5, 1)
    assert R.out_hw(9, 67, 5, 2) == (5, 34) and R.out_hw(7, 66, 3, 2) == (4, 33) and R.out_hw(9, 33, 2, 1) == (9, 33)


def test_nan_activation_has_atens_footprint_also_under_zero_weights():
    x = torch.randn(1, 6, 7, 8, dtype=torch.float64)
    x[0, 2, 3, 1] = float("nan")
    w = torch.randn(4, 8, 3, 3, dtype=torch.float64)
    w[1] = 0                                                   # 0 * NaN = NaN in ATen and in an MFMA
    for stride in (1, 2):
        got, want = R.conv2d(x, w, k=3, stride=stride).y, _aten(x, w, 3, stride)
        assert torch.equal(torch.isnan(got), torch.isnan(want)) and int(torch.isnan(got).sum()) == (36 if stride == 1 else 8)


def test_k2_parity_layers_assemble_the_transposed_conv():
    """The four k2 launches with ops.deconv2d_parity_weights (the weight tensors only) = float64 ConvTranspose2d(k3, s2, p1, op1)."""
    from wild_deep_mvs_amd import ops
    g = torch.Generator().manual_seed(3)
    for B, Hi, Wi, ci, co in [(2, 1, 1, 8, 4), (1, 5, 4, 16, 8), (2, 3, 7, 8, 12)]:
        x = torch.randn(B, Hi, Wi, ci, generator=g, dtype=torch.float64)
        wt = torch.randn(ci, co, 3, 3, generator=g)
        sub = ops.deconv2d_parity_weights(wt)
        out = torch.full((B, 2 * Hi, 2 * Wi, co + 4), 7.0, dtype=torch.float64)
        for p in range(4):
            assert tuple(sub[p].shape) == (co, ci, 2, 2)
            out = R.place(R.conv2d(x, sub[p], k=2, stride=1).y, out, 4, p)
        want = F.conv_transpose2d(_nchw(x), wt.double(), stride=2, padding=1, output_padding=1).permute(0, 2, 3, 1)
        torch.testing.assert_close(out[..., 4:], want, rtol=0, atol=1e-12 * float(want.abs().max()))
        assert bool((out[..., :4] == 7.0).all())               # channels outside the slice keep what the map held


def _unpack(packed, c_pad, c_out, k, dtype):
    """ops.pack_conv2d_weights' uint16 array -> A [16 tiles, 32 steps] float64 by the kernel's index map: lane (m = lane & 15,
    g = lane >> 4), element j of step s and tile t holds output channel 16 t + m and k = 32 s + 8 g + j."""
    nt, nsteps = (c_out + 15) // 16, (k * k * c_pad + 31) // 32
    bits = np.asarray(packed, dtype=np.uint16).reshape(nsteps, nt, 64, 8)
    val = bits.view(np.float16).astype(np.float64) if dtype == torch.float16 else (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    A = np.zeros((nt * 16, nsteps * 32))
    for lane in range(64):
        m, g_ = lane & 15, lane >> 4
        for j in range(8):
            A[m::16, 8 * g_ + j::32] = val[:, :, lane, j].T          # [tile, step]
    return A


def _contract_like_the_kernel(A, x, c_pad, k, stride):
    """out[co, pixel] = sum_k A[co, k] X[k, pixel], X built as conv2d_kernel reads its brick: k = tap * c_in_padded + ci, tap =
    kh * k + kw at input (stride * o + kh - pad, stride * o + kw - pad), zero outside the map; the k padding re-reads the LAST tap."""
    B, Hi, Wi, _ = x.shape
    lo, hi = R.geometry(k, stride)
    Ho, Wo = R.out_hw(Hi, Wi, k, stride)
    xp = np.zeros((B, Hi + lo + hi, Wi + lo + hi, c_pad))
    xp[:, lo:lo + Hi, lo:lo + Wi] = x
    X = np.zeros((A.shape[1], B, Ho, Wo))
    for kk in range(A.shape[1]):
        tap, ci = min(kk // c_pad, k * k - 1), kk % c_pad
        kh, kw = tap // k, tap % k
        X[kk] = xp[:, kh:kh + stride * (Ho - 1) + 1:stride, kw:kw + stride * (Wo - 1) + 1:stride, ci]
    return np.einsum("ok,kbhw->bhwo", A, X)


PACK_LAYERS = sorted({(c.c_in, c.c_pad, c.c_out, c.k, c.stride) for c in R.CASES} | {(3, 8, 8, 3, 1), (16, 16, 20, 3, 1), (3, 8, 20, 5, 2)})


@pytest.mark.parametrize("dt", list(R.DTYPES))
@pytest.mark.parametrize("ci,cpad,co,k,stride", PACK_LAYERS)
def test_host_packer_contracts_like_the_kernel(ci, cpad, co, k, stride, dt):
    L, ops = _engine()
    dtype = R.DTYPES[dt]
    g = torch.Generator().manual_seed(ci * 1000 + co * 10 + k)
    w = torch.randn(co, ci, k, k, generator=g)
    A = _unpack(ops.pack_conv2d_weights(w, cpad, dtype), cpad, co, k, dtype)
    wr = w.to(dtype).double()
    # layout: real entries are the rounded weights, every padded k entry, padded input channel and padded output channel is exactly 0
    want = np.zeros_like(A)
    full = np.zeros((co, k * k, cpad))
    full[:, :, :ci] = wr.reshape(co, ci, k * k).permute(0, 2, 1).numpy()
    want[:co, :k * k * cpad] = full.reshape(co, -1)
    assert np.array_equal(A, want)
    x = torch.zeros(2, 4, 5, cpad, dtype=torch.float64)
    x[..., :ci] = torch.randn(2, 4, 5, ci, generator=g, dtype=torch.float64)
    x[..., ci:] = 3.0                                          # (what the padded channels hold is multiplied by exact zeros)
    got = _contract_like_the_kernel(A, x.numpy(), cpad, k, stride)
    ref = R.conv2d(x, wr, k=k, stride=stride).y.numpy()
    assert not got[..., co:].any()
    np.testing.assert_allclose(got[..., :co], ref, rtol=0, atol=1e-12 * np.abs(ref).max())


def test_k3_parity_layers_assemble_the_input_gradient_of_k5_s2():
    """The four k3 s1 parity layers of training._dgrad2d_k5s2_layers (their weights read back out of the packed layers with the
    kernel's index map) assemble the float64 autograd input gradient of a k5 s2 p2 conv on an even-sized input; and the index map
    restated here, k = a + 2 - 2 m for tap m = -1, 0, +1 of parity a, gives the same weights."""
    L, ops = _engine()
    from wild_deep_mvs_amd import training
    g = torch.Generator().manual_seed(11)
    co, ci, B, Hi, Wi = 16, 8, 2, 6, 10
    w = torch.randn(co, ci, 5, 5, generator=g).to(torch.bfloat16).float()            # exact in both storage types
    layers = training._dgrad2d_k5s2_layers(w, torch.float16)
    x = torch.randn(B, ci, Hi, Wi, generator=g, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x, w.double(), stride=2, padding=2)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    (want,) = torch.autograd.grad(y, x, dy)
    dx = torch.full((B, Hi, Wi, ci), float("nan"), dtype=torch.float64)
    for p, layer in enumerate(layers):
        assert (layer.c_in, layer.c_out, layer.ks, layer.stride) == (co, ci, 3, 1)
        A = _unpack(layer.packed.view(torch.int16).numpy().view(np.uint16), co, ci, 3, torch.float16)
        wp = torch.from_numpy(A[:ci, :9 * co].reshape(ci, 3, 3, co)).permute(0, 3, 1, 2).contiguous()      # [ci,co,3,3]
        a, b = p >> 1, p & 1
        mine = torch.zeros(ci, co, 3, 3, dtype=torch.float64)
        for ty in range(3):
            for tx in range(3):
                ky, kx = a + 2 - 2 * (ty - 1), b + 2 - 2 * (tx - 1)
                if 0 <= ky <= 4 and 0 <= kx <= 4:
                    mine[:, :, ty, tx] = w[:, :, ky, kx].double().t()
        assert torch.equal(wp, mine)
        dx = R.place(R.conv2d(dy.permute(0, 2, 3, 1), wp, k=3, stride=1).y, dx, 0, p)
    torch.testing.assert_close(dx, want.permute(0, 2, 3, 1), rtol=0, atol=1e-12 * float(want.abs().max()))


def test_epilogue_order_and_non_finite_table():
    g = torch.Generator().manual_seed(4)
    B, Hi, Wi, ci, co = 2, 5, 6, 8, 12
    x = torch.randn(B, Hi, Wi, ci, generator=g).to(torch.bfloat16)
    w = torch.randn(co, ci, 3, 3, generator=g).to(torch.bfloat16).float()
    bn = (torch.rand(co, generator=g) + 0.5, torch.randn(co, generator=g), torch.randn(co, generator=g), torch.rand(co, generator=g) + 0.5)
    cb = torch.randn(co, generator=g)
    skip = torch.randn(B, Hi, Wi, co + 8, generator=g).to(torch.bfloat16)
    conv = F.conv2d(_nchw(x.double()), w.double(), cb.double(), padding=1)
    # BN folded as Conv2dLayer.build folds it (fp32 vectors), the skip BEFORE the activation (BasicBlock: relu(bn(conv) + shortcut))
    scale, bias = R.fold_bn(*bn, conv_bias=cb)
    want = F.relu(F.batch_norm(conv, bn[2].double(), bn[3].double(), bn[0].double(), bn[1].double(), False, 0.0, 1e-5) + _nchw(skip[..., 4:4 + co].double()))
    r = R.conv2d(x, w, k=3, stride=1, scale=scale, bias=bias, skip=skip, skip_coff=4, neg_slope=0.0)
    torch.testing.assert_close(_nchw(r.y), want, rtol=0, atol=4e-6 * float(r.U.max()))      # (the fold is fp32: 2^-24 relative per vector)
    assert float((want == 0).double().mean()) > 0.2 and float((r.v < 0).double().mean()) > 0.2
    try:
        from wild_deep_mvs_amd import ops
        layer = ops.Conv2dLayer.build(w, stride=1, device="cpu", bn=bn, conv_bias=cb, relu=True, dtype=torch.bfloat16)
    except Exception:                                          # no host library: the fold is still pinned by the line above
        layer = None
    if layer is not None:
        assert torch.equal(layer.scale, scale) and torch.equal(layer.bias, bias) and layer.neg_slope == 0.0
    # bias + LeakyReLU(0.1) (CVP's pyramid), and no activation
    r = R.conv2d(x, w, k=3, stride=1, bias=cb, neg_slope=0.1)
    torch.testing.assert_close(_nchw(r.y), F.leaky_relu(conv, 0.1), rtol=0, atol=1e-12)
    torch.testing.assert_close(_nchw(R.conv2d(x, w, k=3, stride=1, bias=cb).y), conv, rtol=0, atol=1e-12)
    # non-finite v: as torch.relu / F.leaky_relu / the identity
    v = torch.tensor([float("nan"), -INF, INF, -2.0, 0.0, -0.0, 3.0], dtype=torch.float64)
    for slope, want in ((0.0, F.relu(v)), (0.1, F.leaky_relu(v, 0.1)), (1.0, v)):
        got = R.activation(v, slope)
        assert torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(got[1:], want[1:]), slope
    assert float(R.activation(v, 0.0)[1]) == 0.0 and float(R.activation(v, 0.1)[1]) == -INF
    # through the whole reference: a NaN / -inf / +inf skip element
    sk = torch.zeros(B, Hi, Wi, co)
    sk[0, 0, 0, 0], sk[0, 0, 0, 1], sk[0, 0, 0, 2] = float("nan"), -INF, INF
    for slope, at_ninf in ((0.0, 0.0), (0.1, -INF), (1.0, -INF)):
        y = R.conv2d(x, w, k=3, stride=1, skip=sk, neg_slope=slope).y
        assert bool(torch.isnan(y[0, 0, 0, 0])) and float(y[0, 0, 0, 1]) == at_ninf and float(y[0, 0, 0, 2]) == INF and int(torch.isnan(y).sum()) == 1


def test_round16_models_the_engines_stores():
    f16, bf16 = torch.float16, torch.bfloat16
    v = torch.tensor([65504.0, 65519.9, 65520.0, 1e6, INF, -65519.9, -65520.0, -INF, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 2.0 ** -25, 2.0 ** -24 * 1.5, -0.0])
    want = torch.tensor([65504.0, 65504.0, 65504.0, 65504.0, 65504.0, -65504.0, -65504.0, -65504.0, 1.0, 1.0 + 2.0 ** -9, 0.0, 2.0 ** -23, -0.0])
    for src in (v, v.double()):
        got = R.round16(src, f16)
        assert got.dtype == f16 and torch.equal(got.double(), want.double()) and bool(torch.signbit(got[-1]))
    assert bool(torch.isnan(R.round16(torch.tensor([float("nan")]), f16))) and bool(torch.isnan(R.round16(torch.tensor([float("nan")]), bf16)))
    b = R.round16(torch.tensor([INF, -INF, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 3.0e38, 3.4e38]), bf16)
    assert torch.equal(b.double(), torch.tensor([INF, -INF, 1.0, 1.0 + 2.0 ** -6, 2.0 ** 127 * 1.765625, INF], dtype=torch.float64))
    # the host conversions of pscv_common.h (what pscv_pack_conv2d_weights stores, the software twin of the kernels' packs) agree
    from wild_deep_mvs_amd import _lib as L, ops
    if not os.path.exists(L.LIB_PATH):                         # (the table above holds without the host library)
        return
    g = torch.Generator().manual_seed(8)
    r = torch.cat([v[~torch.isinf(v)], torch.randn(4000, generator=g) * torch.logspace(-9, 5, 4000)])
    for dtype in (f16, bf16):
        w = torch.zeros(len(r) + (-len(r)) % 16, 8, 1, 1)
        w[:len(r), 0, 0, 0] = r
        A = _unpack(ops.pack_conv2d_weights(w, 8, dtype), 8, w.shape[0], 1, dtype)
        assert np.array_equal(A[:len(r), 0], R.round16(r, dtype).double().numpy()), dtype


def _rc(c_in=16, c_out=16, ks=3, stride=1, parity=-1, dtype=None, out_dtype=None, out_cs=None, out_co=0, skip=None, skip_cs=0, skip_co=0, slope=0.0,
        dims=(1, 8, 8)):
    """pscv_conv2d_ex with fake non-null pointers (never dereferenced on the host) -> (rc, error text)."""
    L, _ = _engine()
    lib = L.lib()
    dtype = L.F16 if dtype is None else dtype
    rc = lib.pscv_conv2d_ex(64, dtype, 64, None, None, skip, skip_cs, skip_co, 128, c_out if out_cs is None else out_cs, out_co,
                            dtype if out_dtype is None else out_dtype, *dims, c_in, c_out, ks, stride, parity, slope, None)
    return rc, lib.pscv_last_error().decode()


@pytest.mark.parametrize("kwargs, reasons", [
    (dict(c_in=24, c_out=16), ("unsupported layer c_in=24 c_out=16 k=3 stride=1",)),
    (dict(c_in=8, c_out=16, ks=1), ("unsupported layer c_in=8 c_out=16 k=1 stride=1",)),
    (dict(c_in=16, c_out=16, ks=3, stride=2), ("unsupported layer c_in=16 c_out=16 k=3 stride=2",)),
    (dict(c_in=16, c_out=16, ks=5, stride=1), ("supported layers are", "got k5 s1")),
    (dict(c_in=16, c_out=16, ks=4, stride=1), ("supported layers are", "got k4 s1")),
    (dict(c_in=64, c_out=96), ("c_out=96 above 64 must be a multiple of 64",)),
    (dict(c_in=16, c_out=18), ("c_out=18 must be a multiple of 4",)),
    (dict(c_in=64, c_out=32, ks=2), ("a k2 sub-convolution needs parity 0..3",)),
    (dict(c_in=32, c_out=64, ks=3, stride=2, parity=1), ("an output parity (0..3) only applies to the stride-1 k2 / k3",)),
    (dict(c_in=16, c_out=32, ks=5, stride=2, parity=0), ("an output parity (0..3) only applies to the stride-1 k2 / k3",)),
    (dict(c_in=64, c_out=32, ks=2, parity=4), ("an output parity (0..3) only applies",)),
    (dict(out_cs=24, out_co=12), ("bad output channel slice",)),                     # overruns its stride
    (dict(out_cs=32, out_co=6), ("bad output channel slice",)),                      # off a multiple of 4
    (dict(out_cs=30), ("bad output channel slice",)),
    (dict(skip=64, skip_cs=24, skip_co=12), ("bad skip channel slice",)),
    (dict(skip=64, skip_cs=32, skip_co=2), ("bad skip channel slice",)),
    (dict(skip=64, skip_cs=18), ("bad skip channel slice",)),
    (dict(slope=-0.1), ("neg_slope=-0.1 outside [0,1]",)),
    (dict(slope=1.5), ("neg_slope=1.5 outside [0,1]",)),
    (dict(dtype=0), ("storage dtype 0 must be bf16 or fp16",)),
    (dict(out_dtype=1), ("out dtype 1 must be the storage dtype or fp32",)),         # fp16 in, bf16 out
    (dict(dims=(1, 0, 8)), ("bad sizes",)),
])
def test_conv2d_rejects_before_any_launch(kwargs, reasons):
    """The argument checks of pscv_conv2d_ex and of the dispatcher behind it name the entry point and the reason, and come before
    any HIP call (this machine has no device: a launch attempt would report a HIP error instead)."""
    rc, msg = _rc(**kwargs)
    assert rc == -1 and "pscv_conv2d" in msg and all(r in msg for r in reasons), (rc, msg)


def test_case_table_covers_the_dispatch_table():
    """Every PSCV_C2(ci, nt, k, s) line and every c2w_launch<H, NT, CIN> line of csrc/conv2d.hip is reached by a case of the table
    the GPU file runs: a new instantiation without a case fails here."""
    src = open(os.path.join(REPO, "wild_deep_mvs_amd", "csrc", "conv2d.hip")).read()
    stream = {tuple(int(v) for v in m) for m in re.findall(r"PSCV_C2\((\d+), (\d+), (\d+), (\d+)\)", src)}
    wlds = {tuple(int(v) for v in m) for m in re.findall(r"return c2w_launch<H, (\d+), (\d+)>\(a, st\);", src)}
    assert len(stream) == len(re.findall(r"PSCV_C2\(\d", src)) >= 21 and len(wlds) == len(re.findall(r"return c2w_launch<", src)) >= 4
    have_stream = {R.instantiation(c) for c in R.STREAM_CASES}
    have_wlds = {R.instantiation(c) for c in R.WLDS_CASES}
    assert stream - have_stream == set(), f"PSCV_C2 instantiations without a case: {sorted(stream - have_stream)}"
    assert have_stream - stream == set(), f"cases the dispatcher would reject: {sorted(have_stream - stream)}"
    assert wlds == have_wlds, (wlds, have_wlds)
    # what else the GPU file relies on: the k3 parity layers, 128 output channels, c_out off the tile, unique names
    assert any(c.parity and c.k == 3 for c in R.CASES) and sum(c.c_out == 128 for c in R.CASES) >= 3
    assert {c.c_out for c in R.CASES} >= {8, 20} and len({c.name for c in R.CASES}) == len(R.CASES)
    for c in R.STREAM_CASES:
        want = R.PAR_SIZES if c.parity else (R.S1_SIZES if c.stride == 1 else R.S2_SIZES)
        assert c.sizes == want and {R.batch_of(i) for i in range(len(c.sizes))} == {2, 3}
    eps = [R.epilogue_of(R.CASES.index(c), si) for c in R.STREAM_CASES for si in range(len(c.sizes))]
    assert abs(eps.count("bn_relu") / len(eps) - 0.5) < 0.05 and abs(eps.count("bias_leaky") / len(eps) - 0.25) < 0.05
    assert [R.tall_rows(c) for c in R.WLDS_CASES] == [1035, 1035, 2059, 2059] and R.tall_rows(R.WLDS_CASES[2], 64) == 1019


def _launch_shapes(c):
    if c.kernel == "wlds":
        yield (0,) + R.WLDS_RAGGED
        yield (1, 1, 27, R.TALL_W)              # (three bands' worth of the tall map: same operand statistics)
    else:
        for si, (Hi, Wi) in enumerate(c.sizes):
            yield si, R.batch_of(si), Hi, Wi


@pytest.mark.parametrize("c", R.CASES, ids=lambda c: c.name)
def test_operands_of_every_case_meet_the_conditions_of_the_bounds(c):
    """U > 0 at every output element (the per-element bound is a ratio to U), no non-finite reference value, and max |v| below
    65504 (the 16-bit outputs of the ordinary cases do not saturate; the saturation test sets its own scale)."""
    ci = R.CASES.index(c)
    for dt, dtype in R.DTYPES.items():
        for si, B, Hi, Wi in _launch_shapes(c):
            for p in ((0, 1, 2, 3) if c.parity else (-1,)):
                o = R.make_operands(c, dtype, B, Hi, Wi, epilogue=R.epilogue_of(ci, si), parity=p)
                assert o["x"].dtype == dtype and not o["x"][..., c.c_in:].any() and torch.equal(o["w"], o["w"].to(dtype).float())
                skip = o["skip"] if p < 0 else o["skip"][:, p >> 1::2, p & 1::2]
                for sk in (None, skip):
                    r = R.conv2d(o["x"], o["w"], k=c.k, stride=c.stride, scale=o["scale"], bias=o["bias"], skip=sk, neg_slope=o["neg_slope"])
                    assert bool(torch.isfinite(r.y).all()) and bool(torch.isfinite(r.U).all()), (c.name, dt, Hi, Wi)
                    assert float(r.U.min()) > 0 and float(r.v.abs().max()) < 1000 < R.F16_MAX, (c.name, dt, Hi, Wi)
                    assert r.K == R.k_terms(c.k, c.c_pad)
