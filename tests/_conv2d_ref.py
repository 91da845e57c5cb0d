"""Float64 reference of the 2-D convolution family (csrc/conv2d.hip: pscv_conv2d / pscv_conv2d_ex, ops.conv2d), written from the
definition in include/pscv.h, and the case table that tests/test_conv2d_ref_cpu.py (no GPU) and tests/test_gpu_conv2d_ref.py share.
Nothing here calls into ``ops`` or ``training``.

    v[b,i,j,c] = scale[c] * sum_{ky,kx,ci} w[c,ci,ky,kx] x[b, s i + ky - p, s j + kx - p, ci] + bias[c] (+ skip[b,i,j,c])
    y = v for v >= 0, neg_slope * v below          (torch semantics for non-finite v: NaN stays NaN, relu(-inf) = 0,
                                                    leaky(-inf) = -inf, neg_slope 1 is the identity)

Layers: k3 s1|s2 p1, k5 s2 p2, k1 s1|s2 p0, and k2 p0 with taps (i + ty, j + tx) (the parity sub-convolutions of a stride-2
transposed conv; the row / column past the input is zero).  With ``parity`` p the output pixel (i, j) is pixel
(2 i + (p >> 1), 2 j + (p & 1)) of a [B, 2 Hi, 2 Wi, *] map (``place``).

Error unit: U = |scale| (|w| conv |x|) + |bias| + |skip| per output element.  An fp32 chain that sums the K exact products of
16-bit operands in ANY order and then applies the epilogue's three roundings (fma with scale and bias, the skip add, the slope
product) is within (K + 3) 2^-24 U of ``v`` to first order: (K - 1) 2^-24 for the sum (each partial sum is bounded by
|w| conv |x|), 3 more for the epilogue; K = 32 ceil(k k c_in_padded / 32) counts the zero terms of the k padding too.  The
activation is 1-Lipschitz, so the bound holds for ``y``."""
import collections
import math

import torch

F16_MAX = 65504.0
Ref = collections.namedtuple("Ref", "y v U K")      # y, v, U: float64 [B,Ho,Wo,c_out]


def geometry(k, stride):
    """(pad before, pad after) of a supported (k, stride); raises for the others."""
    if (k, stride) not in ((3, 1), (3, 2), (5, 2), (1, 1), (1, 2), (2, 1)):
        raise ValueError(f"no such layer: k{k} s{stride}")
    return (0, 1) if k == 2 else (k // 2, k // 2)


def out_hw(Hi, Wi, k, stride):
    lo, hi = geometry(k, stride)
    return (Hi + lo + hi - k) // stride + 1, (Wi + lo + hi - k) // stride + 1


def k_terms(k, c_in_padded):
    return 32 * math.ceil(k * k * c_in_padded / 32)


def _taps(x, w, k, stride):
    """sum_{taps, ci} w x -> [B,Ho,Wo,c_out] float64; x [B,Hi,Wi,>=c_in] float64 (channels past c_in are not read), w float64."""
    B, Hi, Wi, _ = x.shape
    c_out, c_in = w.shape[:2]
    lo, hi = geometry(k, stride)
    Ho, Wo = out_hw(Hi, Wi, k, stride)
    xp = torch.zeros(B, Hi + lo + hi, Wi + lo + hi, c_in, dtype=torch.float64)
    xp[:, lo:lo + Hi, lo:lo + Wi] = x[..., :c_in]
    acc = torch.zeros(B, Ho, Wo, c_out, dtype=torch.float64)
    for ky in range(k):
        for kx in range(k):
            xs = xp[:, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride]
            acc += xs @ w[:, :, ky, kx].t()      # (a float64 matrix product keeps 0 * NaN = NaN: pinned against ATen on the CPU)
    return acc


def activation(v, neg_slope):
    if neg_slope == 1.0:
        return v.clone()
    if neg_slope == 0.0:
        return torch.where(v < 0, torch.zeros_like(v), v)           # NaN < 0 is false: NaN stays
    return torch.where(v < 0, v * neg_slope, v)


def conv2d(x, w, *, k, stride, scale=None, bias=None, skip=None, skip_coff=0, neg_slope=1.0):
    """x [B,Hi,Wi,c_in_padded] in the storage type (or any float tensor holding such values), w [c_out,c_in,k,k] rounded to the
    storage type, scale / bias [c_out], skip [B,Ho,Wo,*] read at ``skip_coff`` -> Ref.  ``place`` puts ``y`` into a wider map."""
    assert x.dim() == 4 and w.dim() == 4 and w.shape[2] == w.shape[3] == k and w.shape[1] <= x.shape[3]
    xd, wd = x.double(), w.double()
    c_out = w.shape[0]
    s = _taps(xd, wd, k, stride)
    U = _taps(xd.abs(), wd.abs(), k, stride)
    if scale is not None:
        s = s * scale.double()
        U = U * scale.double().abs()
    if bias is not None:
        s = s + bias.double()
        U = U + bias.double().abs()
    if skip is not None:
        sk = skip[..., skip_coff:skip_coff + c_out].double()
        assert sk.shape == s.shape, (sk.shape, s.shape)
        s = s + sk
        U = U + sk.abs()
    return Ref(activation(s, float(neg_slope)), s, U, k_terms(k, x.shape[3]))


def place(y, into, out_coff=0, parity=-1):
    """``into`` with ``y`` written at channels [out_coff, out_coff + c_out) of every pixel (parity < 0: ``into`` is [B,Ho,Wo,*]) or
    of the pixels (2 i + (parity >> 1), 2 j + (parity & 1)) of a [B,2 Hi,2 Wi,*] map; everything else keeps what ``into`` held."""
    out = into.clone()
    c = y.shape[3]
    assert 0 <= out_coff and out_coff + c <= out.shape[3]
    if parity < 0:
        assert out.shape[:3] == y.shape[:3]
        out[..., out_coff:out_coff + c] = y.to(out.dtype)
    else:
        assert 0 <= parity < 4 and out.shape[1] == 2 * y.shape[1] and out.shape[2] == 2 * y.shape[2]
        out[:, parity >> 1::2, parity & 1::2, out_coff:out_coff + c] = y.to(out.dtype)
    return out


def round16(y, dtype):
    """The engine's 16-bit store of ``y`` (fp32 or float64): round to nearest even; fp16 saturates at +-65504, true inf included
    (pscv_common.h: f32_to_f16_bits / pack_f16x2); bf16 as torch.to(bfloat16); NaN stays NaN."""
    r = y.to(dtype)
    if dtype == torch.float16:
        r = torch.where(torch.isinf(r), torch.copysign(torch.full_like(r, F16_MAX), r), r)
    return r


def fold_bn(gamma, beta, mean, var, eps=1e-5, conv_bias=None):
    """(scale, bias) of an eval-mode BatchNorm2d behind the conv, fp32, in the operation order of ops.Conv2dLayer.build."""
    scale = gamma.float() / torch.sqrt(var.float() + eps)
    bias = beta.float() - mean.float() * scale
    if conv_bias is not None:
        bias = bias + scale * conv_bias.float()
    return scale, bias


# ------------------------------------------------------------------------------------------------------------------------------
# The case table.  ``kernel``: "stream" = conv2d_kernel (PSCV_C2 instantiation (c_in_padded, min(tiles, 4), k, stride)),
# "wlds" = conv2d_wlds_kernel (instantiation (tiles, c_in)); ``parity``: the four parity launches fill one [B,2 Hi,2 Wi,*] map.
# ------------------------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "name kernel c_in c_pad c_out k stride parity sizes")

S1_SIZES = [(1, 1), (3, 5), (9, 33), (13, 47)]         # 8 x 32 tiles: (9, 33) = 2 x 2 tiles, the last one pixel wide
S2_SIZES = [(1, 1), (2, 2), (7, 66), (9, 67)]          # 4 x 32 output pixels: outputs 33 and 34 wide
PAR_SIZES = [(1, 1), (9, 33)]
WLDS_RAGGED = (2, 45, 70)
TALL_W = 97                                            # four column tiles: left border, two interior, one pixel wide


def _stream(c_in, c_out, k, stride, parity=False, note=""):
    c_pad = (c_in + 7) // 8 * 8
    sizes = PAR_SIZES if parity else (S1_SIZES if stride == 1 else S2_SIZES)
    name = f"{c_in}to{c_out}k{k}s{stride}" + ("par" if parity else "") + note
    return Case(name, "stream", c_in, c_pad, c_out, k, stride, parity, sizes)


CASES = [
    # every PSCV_C2 line of c2_dispatch, in its order
    _stream(3, 16, 3, 1), _stream(16, 16, 3, 1), _stream(32, 32, 3, 1), _stream(16, 32, 3, 1), _stream(32, 16, 3, 1),
    _stream(3, 64, 3, 1), _stream(64, 64, 3, 1), _stream(64, 32, 3, 1),
    _stream(32, 64, 3, 1),
    _stream(8, 16, 5, 2), _stream(16, 32, 5, 2), _stream(8, 32, 5, 2), _stream(16, 16, 5, 2),
    _stream(16, 32, 1, 1), _stream(32, 64, 1, 2), _stream(64, 128, 1, 2),                  # 128 out: two blockIdx.y halves
    _stream(32, 64, 3, 2), _stream(64, 128, 3, 2),
    _stream(128, 128, 3, 1), _stream(128, 32, 3, 1),
    _stream(128, 64, 2, 1, parity=True), _stream(64, 32, 2, 1, parity=True),
    # k3 s1 with a parity: the data gradient of the k5 s2 layers 8 -> 16 and 16 -> 32
    _stream(16, 8, 3, 1, parity=True), _stream(32, 16, 3, 1, parity=True),
    # c_out off the 16-channel tile (the `c0 >= cout` guard of the direct epilogue), the first layer as MVSNet has it (3 -> 8)
    _stream(16, 20, 3, 1), _stream(3, 8, 3, 1), _stream(64, 64, 1, 2),
    # the persistent weights-in-LDS kernel (sizes: the ragged map of WLDS_RAGGED and the tall map of tall_rows())
    Case("wlds64to64", "wlds", 64, 64, 64, 3, 1, False, []), Case("wlds64to32", "wlds", 64, 64, 32, 3, 1, False, []),
    Case("wlds32to32", "wlds", 32, 32, 32, 3, 1, False, []), Case("wlds32to16", "wlds", 32, 32, 16, 3, 1, False, []),
]
STREAM_CASES = [c for c in CASES if c.kernel == "stream"]
WLDS_CASES = [c for c in CASES if c.kernel == "wlds"]
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}


def instantiation(c):
    """The template arguments the dispatcher picks for the case: (c_in_padded, tiles per workgroup, k, stride) or (tiles, c_in)."""
    nt = (c.c_out + 15) // 16
    return (nt, c.c_pad) if c.kernel == "wlds" else (c.c_pad, min(nt, 4), c.k, c.stride)


def batch_of(size_index):
    """B = 2 and B = 3 alternate over a case's sizes: the workgroup count is not always a multiple of 8."""
    return 2 + size_index % 2


def epilogue_of(case_index, size_index):
    """Folded BN + ReLU on half of the (case, size) pairs, bias + LeakyReLU(0.1) on a quarter, no activation on the rest."""
    return ("bn_relu", "bn_relu", "bias_leaky", "none")[(case_index + size_index) % 4]


def tall_rows(c, n_cu=256):
    """Rows of the tall B = 1, Wi = 97 map (four column tiles) on which every persistent workgroup takes a second tile, some a
    third: 4 ceil(Hi / 8) >= 2 grid + 3 tiles, grid = n_cu x workgroups per CU (2 while weights + brick + rows fit 80 KiB of LDS);
    at least 512 tiles, so that the default knob (conv2d_wlds = 1) takes this kernel too."""
    nt = c.c_out // 16
    lds = 9 * (c.c_in // 32) * nt * 1024 + 10 * 34 * c.c_in * 2 + 8 * 32 * (nt * 32 + 16)
    grid = n_cu * (2 if lds <= 80 * 1024 else 1)
    return max(8 * math.ceil((2 * grid + 3) / 4) + 3, 8 * 127 + 3)


def make_operands(c, dtype, B, Hi, Wi, *, epilogue="none", parity=-1, seed=0, with_skip=True):
    """CPU operands of one launch of case ``c``: x [B,Hi,Wi,c_pad] in ``dtype`` (channels past c_in zero), w fp32 [c_out,c_in,k,k]
    holding ``dtype`` values, bn (gamma, beta, mean, var) or None, conv_bias or None, (scale, bias) fp32 as the layer folds them,
    skip [B,Hs,Ws,c_out] in ``dtype`` (Hs, Ws: the full output map, 2 Hi x 2 Wi with a parity), neg_slope."""
    g = torch.Generator().manual_seed(1000003 * (CASES.index(c) + 1) + 7919 * Hi + 131 * Wi + 17 * (parity + 1) + seed)
    x = torch.zeros(B, Hi, Wi, c.c_pad)
    x[..., :c.c_in] = torch.randn(B, Hi, Wi, c.c_in, generator=g)
    w = (torch.randn(c.c_out, c.c_in, c.k, c.k, generator=g) / (c.c_in * c.k * c.k) ** 0.5).to(dtype).float()
    bn = conv_bias = scale = bias = None
    neg_slope = 1.0
    if epilogue == "bn_relu":
        bn = (torch.rand(c.c_out, generator=g) + 0.5, torch.randn(c.c_out, generator=g) * 0.1, torch.randn(c.c_out, generator=g) * 0.1,
              torch.rand(c.c_out, generator=g) + 0.5)
        scale, bias = fold_bn(*bn)
        neg_slope = 0.0
    elif epilogue == "bias_leaky":
        conv_bias = torch.randn(c.c_out, generator=g) * 0.2
        bias = conv_bias.clone()
        neg_slope = 0.1
    else:
        assert epilogue == "none", epilogue
    Ho, Wo = (2 * Hi, 2 * Wi) if c.parity else out_hw(Hi, Wi, c.k, c.stride)
    skip = torch.randn(B, Ho, Wo, c.c_out, generator=g).to(dtype) if with_skip else None
    return dict(x=x.to(dtype), w=w, bn=bn, conv_bias=conv_bias, scale=scale, bias=bias, skip=skip, neg_slope=neg_slope)
