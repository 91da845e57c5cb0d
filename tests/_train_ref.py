"""Float64 restatements of the training kernels (csrc/train_elem.hip, csrc/fuse.hip, csrc/conv3d_wgrad.hip) and the input
builders their tests share.

Every function takes what the ``ops`` wrapper of the same name takes -- channels-last 16-bit volumes with their values as
they are, fp32 vectors -- lifts it to float64 and evaluates the formula of the header (include/pscv.h) and of the comment
above the kernel, never the kernel's loops.  Functions that feed a tolerance also return ``T``: the same expression with
every term replaced by its absolute value, the yardstick the fp32 rounding error of any evaluation order is bounded against.

tests/test_train_ref_cpu.py holds these against float64 autograd of the torch modules; tests/test_gpu_train_kernels.py holds
the kernels against these.  Both files draw their inputs from the builders at the bottom, so that the conditions checked on
the CPU (exactness of the integer cases, no sign test within rounding of zero, multi-tile plans) hold for what the GPU sees.
"""
import math

import torch

F64 = torch.float64
MANT = {torch.float16: 10, torch.bfloat16: 7}       # stored fraction bits
EMIN = {torch.float16: -14, torch.bfloat16: -126}    # exponent of the smallest normal
U32 = 2.0 ** -24                                     # fp32 unit roundoff


def f64(x):
    return None if x is None else x.detach().to("cpu", F64)


def _exponent(x, dtype):
    """floor(log2 |x|), not below the exponent of the format's smallest normal (subnormals share that spacing)."""
    _, e = torch.frexp(x.abs().clamp(min=2.0 ** (EMIN[dtype] - 1)))
    return (e - 1).clamp(min=EMIN[dtype])


def ulp16(x, dtype):
    """Spacing of ``dtype`` at |x| (float64)."""
    x = f64(x)
    return torch.ldexp(torch.ones_like(x), _exponent(torch.nan_to_num(x, nan=0.0, posinf=0.0, neginf=0.0), dtype) - MANT[dtype])


def round16(x, dtype):
    """x (float64) rounded to ``dtype``, nearest even, ONE rounding (no detour through fp32); returned as float64.  fp16 saturates
    at +-65504 (also for +-inf: the engine's stores never produce inf), bf16 overflows to inf like the hardware convert; NaN stays."""
    x = f64(x)
    fin = torch.nan_to_num(x, nan=0.0, posinf=0.0, neginf=0.0)
    q = torch.ldexp(torch.ones_like(fin), _exponent(fin, dtype) - MANT[dtype])
    r = torch.round(fin / q) * q                     # torch.round: half to even; the scaling by a power of two is exact
    if dtype == torch.float16:
        r = r.clamp(-65504.0, 65504.0)
        r = torch.where(torch.isinf(x), torch.sign(x) * 65504.0, r)
    else:
        big = float(torch.finfo(torch.bfloat16).max)
        r = torch.where(r.abs() > big, torch.sign(r) * math.inf, r)
        r = torch.where(torch.isinf(x), x, r)
    return torch.where(torch.isnan(x), x, r)


def _grouped(y, groups):
    """[..., C] volume -> [groups, voxels per group, C] float64 (the batch axis holds the groups back to back)."""
    y = f64(y)
    return y.reshape(groups, -1, y.shape[-1])


def _rows(v, groups):
    """[C] or [groups, C] per-channel constants -> [groups, 1, C] float64."""
    v = f64(v)
    return (v.reshape(1, 1, -1).expand(groups, 1, -1) if v.dim() == 1 else v.reshape(groups, 1, -1))


def _ngroups(scale):
    return 1 if scale.dim() == 1 else scale.shape[0]


# ---- BatchNorm -------------------------------------------------------------------------------------------------------
def bn_sums(y, groups=1, absolute=False):
    """[groups, 2, C]: per-channel sum and sum of squares of every group (``absolute``: of |y|, for the error bound)."""
    g = _grouped(y, groups)
    if absolute:
        g = g.abs()
    return torch.stack([g.sum(1), (g * g).sum(1)], 1)


def bn_finalize(sums, nvox, gamma, beta, eps, momentum, running=None):
    """sums [groups, 2, C] -> (out [groups, 4, C] = scale, bias, mean, invstd; (running_mean, running_var) after one update per
    group, in order).  Biased variance clamped at 0 for the normalisation, unbiased (n / max(n - 1, 1)) for the running one."""
    sums = f64(sums)
    sums = sums.reshape(-1, 2, sums.shape[-1])
    C = sums.shape[-1]
    gamma = torch.ones(C, dtype=F64) if gamma is None else f64(gamma)
    beta = torch.zeros(C, dtype=F64) if beta is None else f64(beta)
    rm, rv = (None, None) if running is None else (f64(running[0]).clone(), f64(running[1]).clone())
    out = []
    for s in sums:
        mean = s[0] / nvox
        var = (s[1] / nvox - mean * mean).clamp(min=0.0)
        invstd = 1.0 / torch.sqrt(var + eps)
        scale = gamma * invstd
        out.append(torch.stack([scale, beta - mean * scale, mean, invstd]))
        if rm is not None:
            rm = rm * (1.0 - momentum) + mean * momentum
            rv = rv * (1.0 - momentum) + var * (nvox / max(nvox - 1, 1)) * momentum
    return torch.stack(out), (rm, rv)


def _z(y, scale, bias):
    G = _ngroups(scale)
    return _grouped(y, G), _rows(scale, G), _rows(bias, G)


def relu_near_zero(y, scale, bias):
    """Elements whose sign test z > 0 an fp32 evaluation may decide differently from float64: |z| <= 2^-22 (|y scale| + |bias|)."""
    g, sc, bi = _z(y, scale, bias)
    return ((g * sc + bi).abs() <= 2.0 ** -22 * ((g * sc).abs() + bi.abs())).reshape(f64(y).shape)


def bn_act(y, scale, bias, relu, skip=None):
    """(out, T) of [relu](y scale + bias) + skip; ``relu`` False / True (before the add) / "post" (after it).  NaN propagates
    through the ReLU like torch.relu."""
    g, sc, bi = _z(y, scale, bias)
    z = g * sc + bi
    T = (g * sc).abs() + bi.abs()
    if relu is True:
        z = torch.where(z < 0, torch.zeros_like(z), z)
    if skip is not None:
        s = _grouped(skip, g.shape[0])
        z, T = z + s, T + s.abs()
    if relu == "post":
        z = torch.where(z < 0, torch.zeros_like(z), z)
    shape = f64(y).shape
    return z.reshape(shape), T.reshape(shape)


def _dz(dact, y, scale, bias, relu):
    g, sc, bi = _z(y, scale, bias)
    d = _grouped(dact, g.shape[0])
    if relu:
        d = torch.where(g * sc + bi > 0, d, torch.zeros_like(d))
    return d, g


def bn_bwd_sums(dact, y, scale, bias, relu, absolute=False):
    """[groups, 2, C]: sum dz and sum dz y with dz = dact [y scale + bias > 0] (or dact without the ReLU)."""
    d, g = _dz(dact, y, scale, bias, relu)
    if absolute:
        d, g = d.abs(), g.abs()
    return torch.stack([d.sum(1), (d * g).sum(1)], 1)


def bn_bwd_coeffs(sums, mean, invstd, gamma, nvox):
    """sums [groups, 2, C] -> [groups, 5, C] = ca, cb, cc, d gamma, d beta, with dy = ca dz + cb y + cc the input gradient of
    batch_norm(training=True): dy = gamma invstd (dz - mean(dz) - xhat mean(dz xhat)), xhat = (y - mean) invstd."""
    sums = f64(sums)
    sums = sums.reshape(-1, 2, sums.shape[-1])
    G, _, C = sums.shape
    mean, invstd = f64(mean).reshape(G, C), f64(invstd).reshape(G, C)
    gamma = torch.ones(C, dtype=F64) if gamma is None else f64(gamma)
    dbeta = sums[:, 0]
    dgamma = invstd * (sums[:, 1] - mean * dbeta)
    k = gamma * invstd
    cb = -k * invstd * dgamma / nvox
    cc = -k * dbeta / nvox - cb * mean
    return torch.stack([k.expand(G, C), cb, cc, dgamma, dbeta], 1)


def bn_bwd_apply(dact, y, scale, bias, ca, cb, cc, relu):
    """(dy, T) of ca dz + cb y + cc."""
    d, g = _dz(dact, y, scale, bias, relu)
    G = g.shape[0]
    a, b, c = _rows(ca, G), _rows(cb, G), _rows(cc, G)
    shape = f64(y).shape
    return (a * d + b * g + c).reshape(shape), ((a * d).abs() + (b * g).abs() + c.abs()).reshape(shape)


def relu_bwd(dout, out, slope, dtype):
    """(dpre, stored, sums): dpre = dout (out > 0 ? 1 : slope) with ``slope`` as the fp32 number the ABI receives; ``stored`` =
    dpre rounded to the storage type; sums [C] = per-channel sum of the STORED values (what the header promises)."""
    slope = float(torch.tensor(slope, dtype=torch.float32))
    d, o = f64(dout), f64(out)
    dpre = torch.where(o > 0, d, d * slope)
    stored = round16(dpre, dtype)
    return dpre, stored, stored.reshape(-1, d.shape[-1]).sum(0)


# ---- softmax heads ---------------------------------------------------------------------------------------------------
def softargmin_heads_bwd(logits, depth=None, g_depth=None, g_index=None, g_entropy=None):
    """(d loss / d logits [B,D,h,w], T).  p = softmax over D; heads depth = sum p depth_d, index = sum p d,
    entropy = -sum p log clamp(p, 1e-9, 1); derivative of the clamped log: 1 / p where p > 1e-9, else 0, so
    d entropy / d logit_d = p_d (a_d - sum_k p_k a_k) with a_d = -(log clamp(p_d) + [p_d > 1e-9])."""
    l = f64(logits)
    B, D, h, w = l.shape
    p = torch.softmax(l, 1)
    v = torch.zeros_like(p)
    T = torch.zeros_like(p)

    def head(g, val):
        e = (p * val).sum(1, keepdim=True)
        ea = (p * val.abs()).sum(1, keepdim=True)
        ga = f64(g).unsqueeze(1)
        return ga * (val - e), ga.abs() * (val.abs() + ea)

    if g_depth is not None:
        dep = f64(depth)
        dep = dep.reshape(B, D, 1, 1).expand(B, D, h, w) if dep.dim() == 2 else dep
        a, b = head(g_depth, dep)
        v, T = v + a, T + b
    if g_index is not None:
        a, b = head(g_index, torch.arange(D, dtype=F64).reshape(1, D, 1, 1).expand(B, D, h, w))
        v, T = v + a, T + b
    if g_entropy is not None:
        a, b = head(g_entropy, -(p.clamp(1e-9, 1.0).log() + (p > 1e-9).to(F64)))
        v, T = v + a, T + b
    return p * v, p * T


# ---- visibility-weighted fusion ----------------------------------------------------------------------------------------
def _weights(uncerts):
    w = torch.stack([torch.exp(-f64(u)) for u in uncerts])          # [n,B,h,w]
    return w, w.sum(0)


def fuse(interms, uncerts, normalise=True):
    """(out, wsum, T): sum_v w_v I_v (/ sum_v w_v when ``normalise``), w_v = exp(-uncert_v) per pixel."""
    w, W = _weights(uncerts)
    I = torch.stack([f64(t) for t in interms])                     # [n,B,D,h,w,8]
    ww = w[:, :, None, :, :, None]
    out, T = (I * ww).sum(0), (I.abs() * ww).sum(0)
    if normalise:
        out, T = out / W[:, None, :, :, None], T / W[:, None, :, :, None]
    return out, W, T


def fuse_finish(partial, wsum):
    p = f64(partial)
    return p / f64(wsum)[:, None, :, :, None]


def fuse_bwd(interms, uncerts, grad):
    """(d interm [n,...], d uncert [n,B,h,w], bound term [n,B,h,w]): d I_v = G w_v / W;
    d u_v = -(w_v / W) sum_{d,c} G (I_v - fused); the bound term is (w_v / W) sum |G| |I_v - fused|."""
    w, W = _weights(uncerts)
    I = torch.stack([f64(t) for t in interms])
    G = f64(grad)
    s = w / W
    fused = (I * s[:, :, None, :, :, None]).sum(0)
    dI = G.unsqueeze(0) * s[:, :, None, :, :, None]
    diff = I - fused.unsqueeze(0)
    dU = -s * (G.unsqueeze(0) * diff).sum((2, 5))
    TU = s * (G.abs().unsqueeze(0) * diff.abs()).sum((2, 5))
    return dI, dU, TU


# ---- weight gradient of the 3x3x3 convolutions ---------------------------------------------------------------------------
def wgrad(P, Q, stride, absolute=False):
    """G[a][b][tz,ty,tx] = sum_{n,o} P[n,o,a] Q[n, stride o + t - 1, b] (zero outside Q) -> float64 [ca,cb,3,3,3]: 27 matrix
    products over shifted slices of the zero-padded Q.  P [B,Dp,Hp,Wp,ca], Q [B,s Dp,s Hp,s Wp,cb] channels-last."""
    P, Q = f64(P), f64(Q)
    if absolute:
        P, Q = P.abs(), Q.abs()
    B, Dp, Hp, Wp, ca = P.shape
    cb, s = Q.shape[-1], stride
    assert tuple(Q.shape[:4]) == (B, s * Dp, s * Hp, s * Wp)
    Qp = torch.zeros(B, s * Dp + 2, s * Hp + 2, s * Wp + 2, cb, dtype=F64)
    Qp[:, 1:-1, 1:-1, 1:-1] = Q                        # padded index i <-> Q index i - 1
    Pt = P.reshape(-1, ca).t().contiguous()
    out = torch.empty(ca, cb, 3, 3, 3, dtype=F64)
    for tz in range(3):
        for ty in range(3):
            for tx in range(3):
                sl = Qp[:, tz:tz + s * Dp:s, ty:ty + s * Hp:s, tx:tx + s * Wp:s]
                out[:, :, tz, ty, tx] = Pt @ sl.reshape(-1, cb)
    return out


# =======================================================================================================================
# input builders (shared by the CPU and the GPU file)
# =======================================================================================================================
DT = [torch.bfloat16, torch.float16]
CS = [8, 16, 32, 64, 128]


def gen(*key):
    seed = 17
    for k in key:
        seed = (seed * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def ints(g, shape, lo, hi, dtype):
    """Integer-valued 16-bit tensor, uniform in [lo, hi]."""
    return torch.randint(lo, hi + 1, shape, generator=g).to(dtype)


def pow2(g, shape, lo=-1, hi=1):
    """fp32 +-2^k, k uniform in [lo, hi]."""
    k = torch.randint(lo, hi + 1, shape, generator=g)
    sgn = torch.randint(0, 2, shape, generator=g) * 2 - 1
    return (sgn * torch.ldexp(torch.ones(shape), k)).float()


def half_ints(g, shape, lo=-4, hi=3):
    """fp32 k + 0.5, k uniform in [lo, hi]: never zero, so y * scale + bias (y, scale as above) has an exact, nonzero sign."""
    return torch.randint(lo, hi + 1, shape, generator=g).float() + 0.5


def bn_case(C, nvox, groups, dtype, exact, seed=0):
    """One BatchNorm-shaped input set for a [groups, 1, 1, nvox, C] volume: y, dact, skip (16-bit) and per-group constants as rows
    of [G,4,C] / [G,5,C] tensors the way training.py hands them over (scale, bias = rows 0, 1; ca, cb, cc = rows 0, 1, 2)."""
    g = gen(C, nvox, groups, int(exact), seed, 0 if dtype == torch.bfloat16 else 1)
    shape = (groups, 1, 1, nvox, C)
    if exact:
        y, dact, skip = (ints(g, shape, -4, 4, dtype) for _ in range(3))
        # scale in +-{1, 2}: y * scale is an integer, so z = y * scale + (k + 0.5) is never zero and its sign is exact
        fin = torch.stack([pow2(g, (groups, C), 0, 1), half_ints(g, (groups, C)), torch.zeros(groups, C), torch.ones(groups, C)], 1)
        co = torch.stack([pow2(g, (groups, C)), pow2(g, (groups, C)), half_ints(g, (groups, C)), torch.zeros(groups, C),
                          torch.zeros(groups, C)], 1)
    else:
        y = (torch.randn(shape, generator=g) * 1.5 + 0.3).to(dtype)
        dact, skip = torch.randn(shape, generator=g).to(dtype), torch.randn(shape, generator=g).to(dtype)
        fin = torch.stack([torch.randn(groups, C, generator=g), torch.randn(groups, C, generator=g), torch.zeros(groups, C),
                           torch.ones(groups, C)], 1)
        co = torch.stack([torch.rand(groups, C, generator=g) + 0.5, torch.randn(groups, C, generator=g) * 0.1,
                          torch.randn(groups, C, generator=g) * 0.1, torch.zeros(groups, C), torch.zeros(groups, C)], 1)
    return dict(y=y, dact=dact, skip=skip, fin=fin.contiguous(), co=co.contiguous())


# (C, voxels per group, groups): a single partial block; ragged; every CG instance.  nvox = 3 and 777 are no multiple of 256 chunks.
BN_SMALL = [(C, n, 1) for C in CS for n in (3, 777)]
# more than 1024 * 256 chunks and ragged: every block of the reductions takes a second grid-stride step
RED_MULTI = (64, 40037, 1)
# groups that do not divide 1024, and the 256-group limit (4 blocks per group); every group's 1024 // groups blocks take >= 2 steps
RED_GROUPED = [(8, 2 * 512 * 256 + 77, 2), (16, 204 * 256 + 131, 5), (8, 1024 + 59, 256)]
# just above 8192 * 256 chunks and ragged: the element-wise kernels take a second step (the ~34 MB tensors)
ELEM_MULTI = (64, 262181, 1)
ELEM_GROUPED = [(16, 333, 2), (32, 131, 5)]


def red_geometry(nchunk, groups):
    """(blocks per group, grid-stride steps of the longest lane) of the two-phase reductions, from their documented caps."""
    nb = max(1, min((nchunk + 255) // 256, 1024 // groups))
    return nb, (nchunk + nb * 256 - 1) // (nb * 256)


def red_chain(nchunk, groups, CG):
    """Longest chain of dependent fp32 additions one reduction output passes through: the lane's grid-stride steps (each one
    add or one fused multiply-add), the 256 / CG lanes of its channel group in block_reduce2, then the finishing kernel: a
    thread's rows (ceil(nb / 64) in each of four accumulators, up to 4 more in the tail), 2 to join them, 16 row groups."""
    nb, steps = red_geometry(nchunk, groups)
    return steps + 256 // CG + ((nb + 63) // 64 + 4 + 2 + 16)


def softargmin_case(D, seed=0, per_pixel=False, shift=0.0):
    """B = 2, h = 5, w = 7 (70 pixels = two blocks of 32 and one of 6).  Logits random x 2 with a saturated pixel (+60: the 1e-9
    clamp of the entropy is active) and a pixel of all-equal logits."""
    g = gen(D, seed, 77)
    B, h, w = 2, 5, 7
    logits = torch.round(torch.randn(B, D, h, w, generator=g) * 2 * 1024) / 1024     # multiples of 2^-10: ``shift`` is exact in fp32
    logits[0, D // 3, 0, 0] = 60.0
    logits[1, :, 4, 6] = 0.25
    if per_pixel:
        depth = torch.rand(B, D, h, w, generator=g) + torch.arange(D).float().view(1, D, 1, 1)
    else:
        depth = torch.arange(D).float().view(1, D) * 0.3 + torch.tensor([[2.0], [3.0]])
    gs = [torch.randn(B, h, w, generator=g) for _ in range(3)]
    return dict(logits=(logits + shift).contiguous(), depth=depth.contiguous(), gd=gs[0], gi=gs[1], ge=gs[2])


SOFTARGMIN_D = [1, 5, 8, 9, 24, 33, 192]
FUSE_NSRC = [1, 2, 3, 16]
FUSE_D = [1, 7, 8, 9, 33]


def fuse_case(n_src, D, dtype, exact=False, seed=0):
    """n_src pair volumes [2, D, 5, 7, 8], uncertainties spread over [-8, 8], an upstream gradient.  ``exact``: integers and
    uncertainty 0 (weight exactly 1), so that the un-normalised sums are exact."""
    g = gen(n_src, D, int(exact), seed, 0 if dtype == torch.bfloat16 else 1)
    B, h, w = 2, 5, 7
    shape = (B, D, h, w, 8)
    if exact:
        I = [ints(g, shape, -4, 4, dtype) for _ in range(n_src)]
        U = [torch.zeros(B, h, w) for _ in range(n_src)]
        G = ints(g, shape, -4, 4, dtype)
    else:
        I = [torch.randn(shape, generator=g).to(dtype) for _ in range(n_src)]
        U = [(torch.rand(B, h, w, generator=g) * 16 - 8) for _ in range(n_src)]
        G = torch.randn(shape, generator=g).to(dtype)
    return dict(I=I, U=U, G=G)


# (ca, cb, stride, P grid (B, D, H, W), tag).  The eight template instances of wgrad_kernel: 3-D stride 1 / 2 with one / two
# 16-channel b-tiles, single-plane (D = 1, stride 1) with one / two b-tiles and one / four a-tiles.  "multi-tile": more tiles than
# resident workgroups, so a workgroup carries its accumulators over >= 2 tiles (asserted from pscv_conv3d_wgrad_workspace).
WG_SMALL_GRIDS = [(1, 1, 3, 5), (2, 3, 7, 17), (1, 2, 4, 16)]
WG_PAIRS = [(8, 8, 1), (64, 64, 1), (64, 32, 2), (16, 8, 2), (24, 40, 1), (40, 24, 2), (56, 8, 1), (16, 32, 1)]
WGRAD_CASES = [(ca, cb, s, grid, "small") for (ca, cb, s) in WG_PAIRS for grid in WG_SMALL_GRIDS] + [
    (8, 8, 1, (2, 23, 41, 70), "multi-tile"),        # 3-D stride 1, one b-tile: 1320 tiles
    (64, 64, 1, (2, 7, 21, 37), "multi-tile"),       # 3-D stride 1, two b-tiles: 144 tiles
    (16, 8, 2, (2, 13, 23, 70), "multi-tile"),       # 3-D stride 2, one b-tile: 840 tiles
    (64, 32, 2, (2, 7, 11, 40), "multi-tile"),       # 3-D stride 2, two b-tiles: 144 tiles
    (8, 8, 1, (2, 1, 187, 370), "multi-tile"),       # single plane, one a-tile, one b-tile: 1152 tiles
    (16, 32, 1, (2, 1, 187, 370), "multi-tile"),     # single plane, one a-tile, two b-tiles
    (56, 8, 1, (2, 1, 187, 370), "multi-tile"),      # single plane, four a-tiles (the last half empty), one b-tile
    (64, 32, 1, (2, 1, 187, 370), "multi-tile"),     # single plane, four a-tiles, two b-tiles
    (40, 24, 1, (1, 1, 9, 21), "small"),             # single plane with padded a- and b-tiles, ragged rows
]


def wgrad_tiles(grid, stride):
    """(tile count, k-steps per tile) of the plan in csrc/conv3d_wgrad.hip: tiles of tz x ty x 16 P voxels, 2 x 4 (stride 1), 2 x 2
    (stride 2) or 1 x 8 (single plane, stride 1); a k-step is one MFMA over 32 voxels per wave and tap."""
    B, D, H, W = grid
    tz, ty = (1, 8) if (D == 1 and stride == 1) else ((2, 4) if stride == 1 else (2, 2))
    c = lambda a, b: (a + b - 1) // b
    return B * c(D, tz) * c(H, ty) * c(W, 16), tz * ty * 16 // 32


def store_channels(c):
    """Smallest channel count a channels-last volume may carry (8, 16, 32, 64, 128) that holds ``c`` channels."""
    return next(k for k in (8, 16, 32, 64, 128) if k >= c)


def wgrad_case(ca, cb, stride, grid, dtype, exact, wider=0, seed=0):
    """(P, Q, coff): P [B,D,H,W,*], Q [B,sD,sH,sW,*] -- integers in [-2, 2] (exact) or randn rounded to the storage type -- whose
    operands are the channel slices [coff : coff + c].  Volumes carry 8 / 16 / 32 / 64 / 128 channels, so 24, 40 and 56 channels are
    slices at offset 0 of the next larger tensor (the rest holds data the kernel must not read); ``wider`` = 16: slices at offset 8 of
    tensors at least 16 channels wider."""
    g = gen(ca, cb, stride, *grid, int(exact), wider, seed, 0 if dtype == torch.bfloat16 else 1)
    B, D, H, W = grid
    ps, qs = (B, D, H, W, store_channels(ca + wider)), (B, stride * D, stride * H, stride * W, store_channels(cb + wider))
    coff = 8 if wider else 0
    if exact:
        return ints(g, ps, -2, 2, dtype), ints(g, qs, -2, 2, dtype), coff
    return torch.randn(ps, generator=g).to(dtype), torch.randn(qs, generator=g).to(dtype), coff


def wgrad_ref(P, Q, coff, ca, cb, stride, absolute=False):
    return wgrad(P[..., coff:coff + ca], Q[..., coff:coff + cb], stride, absolute)
