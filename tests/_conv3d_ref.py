"""Float64 reference of the 3x3x3 convolution family (csrc/conv3d*.hip: pscv_conv3d, pscv_conv3d_cat2; ops.conv3d), written from
the definition in include/pscv.h, and the case table that tests/test_conv3d_ref_cpu.py (no GPU) and tests/test_gpu_conv3d_ref.py
share.  Nothing here calls into ``ops``.

    acc[b,z,y,x,c] = sum_{kd,kh,kw,ci} w[c,ci,kd,kh,kw] x[b, s z + kd - 1, s y + kh - 1, s x + kw - 1, ci]      S1 (s = 1), S2 (s = 2, out ceil(n / 2))
                     S1 transposed: the same with flipped taps and swapped channel axes of a [ci,co,3,3,3] weight
                     T2 (ConvTranspose3d k3 s2 p1 op1, out 2 n): output o collects x[i] w[ci,c,k] over o = 2 i - 1 + k per axis
    v = scale[c] * acc + bias[c]
    v = (v < floor_c ? floor_c : v)            with RELU_PRE  (floor_c = floor[c], 0 without a floor tensor; ignored without RELU_PRE)
    v = v + skip[..., skip_coff + c]           with a skip tensor
    y = (v < 0 ? 0 : v)                        with RELU_POST
Non-finite values as in torch: NaN stays NaN (``NaN < f`` is false), relu(-inf) = 0, +inf stays.

Error unit: U = |scale| (|w| conv |x|) + |bias| + |skip| per output element.  An fp32 chain that sums the K exact products of 16-bit
operands in ANY order and then applies the epilogue's three roundings (the fma with scale and bias, the skip add, and one to
spare) stays within (K + 3) 2^-24 U of ``v`` to first order; both clamps are 1-Lipschitz, so the bound holds for ``y``.  K counts
the product terms one output's MFMA chains hold, zero-weight padding included: ``k_terms``."""
import collections
import math

import torch

from _conv2d_ref import F16_MAX, fold_bn, round16      # the engine's 16-bit store and the BN fold are the 2-D family's  # noqa: F401

Ref = collections.namedtuple("Ref", "y v U K")          # y, v (before RELU_POST), U: float64 [B,Do,Ho,Wo,c_out]
INF = float("inf")


def out_dhw(kind, D, H, W):
    if kind == "S1":
        return D, H, W
    if kind == "S2":
        return (D + 1) // 2, (H + 1) // 2, (W + 1) // 2
    if kind == "T2":
        return 2 * D, 2 * H, 2 * W
    raise ValueError(f"no such kind: {kind}")


def gather_weight(w, kind, transposed):
    """[c_out,c_in,3,3,3] float64 in the orientation the tap loops below read: Conv3d weights as they are; a stride-1
    ConvTranspose3d [c_in,c_out,3,3,3] with swapped channel axes and flipped taps; T2 with swapped channel axes (tap k as stored)."""
    w = w.double()
    if kind == "T2":
        assert transposed
        return w.permute(1, 0, 2, 3, 4)
    if transposed:
        assert kind == "S1"
        return w.permute(1, 0, 2, 3, 4).flip(2, 3, 4)
    return w


def _t2_axis(k, n):
    """(output slice, input slice) of tap k along one axis of T2: o = 2 i - 1 + k inside [0, 2 n)."""
    if k == 0:
        return slice(1, 2 * n - 2, 2), slice(1, n)
    return (slice(0, 2 * n, 2), slice(0, n)) if k == 1 else (slice(1, 2 * n, 2), slice(0, n))


def taps(x, kind):
    """Yields ((kd, kh, kw), xs) with xs [B,Do,Ho,Wo,c] float64: the input value tap (kd, kh, kw) multiplies at every output voxel
    (zero where the tap falls outside the volume, or -- T2 -- where the output's parity does not take that tap)."""
    B, D, H, W, c = x.shape
    Do, Ho, Wo = out_dhw(kind, D, H, W)
    if kind == "T2":
        for kd in range(3):
            for kh in range(3):
                for kw in range(3):
                    xs = torch.zeros(B, Do, Ho, Wo, c, dtype=torch.float64)
                    (od, id_), (oh, ih), (ow, iw) = _t2_axis(kd, D), _t2_axis(kh, H), _t2_axis(kw, W)
                    xs[:, od, oh, ow] = x[:, id_, ih, iw]
                    yield (kd, kh, kw), xs
        return
    s = 1 if kind == "S1" else 2
    xp = torch.zeros(B, D + 2, H + 2, W + 2, c, dtype=torch.float64)
    xp[:, 1:D + 1, 1:H + 1, 1:W + 1] = x
    for kd in range(3):
        for kh in range(3):
            for kw in range(3):
                yield (kd, kh, kw), xp[:, kd:kd + s * (Do - 1) + 1:s, kh:kh + s * (Ho - 1) + 1:s, kw:kw + s * (Wo - 1) + 1:s]


def accumulate(x, wg, kind):
    """sum over taps and input channels -> [B,Do,Ho,Wo,c_out] float64; x [B,D,H,W,c_in] float64, wg = gather_weight(...)."""
    acc = None
    for (kd, kh, kw), xs in taps(x, kind):
        t = xs @ wg[:, :, kd, kh, kw].t()       # (a float64 matrix product keeps 0 * NaN = NaN: pinned against ATen on the CPU)
        acc = t if acc is None else acc + t
    return acc


def epilogue(acc, *, scale=None, bias=None, floor=None, skip=None, relu_pre=False, relu_post=False):
    """(y, v) of the definition above from float64 ``acc``; skip already sliced to c_out channels."""
    v = acc
    if scale is not None:
        v = v * scale.double()
    if bias is not None:
        v = v + bias.double()
    if relu_pre:
        fl = torch.zeros(acc.shape[-1], dtype=torch.float64) if floor is None else floor.double()
        v = torch.where(v < fl, fl.expand_as(v), v)                  # NaN < fl is false: NaN stays; fl = -inf is never selected
    if skip is not None:
        v = v + skip.double()
    y = torch.where(v < 0, torch.zeros_like(v), v) if relu_post else v.clone()
    return y, v


def contract(x, w, *, kind, transposed=False):
    """(acc, |w| conv |x|) float64 [B,Do,Ho,Wo,c_out]: the part of the reference that does not depend on the epilogue."""
    wg = gather_weight(w, kind, transposed)
    xd = x[..., :wg.shape[1]].double()
    return accumulate(xd, wg, kind), accumulate(xd.abs(), wg.abs(), kind)


def finish(acc, Uacc, *, scale=None, bias=None, floor=None, skip=None, skip_coff=0, relu_pre=False, relu_post=False, K=0):
    """Ref from ``contract``'s pair: the epilogue on ``acc`` and the same expression on absolute values."""
    c_out = acc.shape[-1]
    U = Uacc
    if scale is not None:
        U = U * scale.double().abs()
    if bias is not None:
        U = U + bias.double().abs()
    sk = None
    if skip is not None:
        sk = skip[..., skip_coff:skip_coff + c_out]
        assert sk.shape == acc.shape, (sk.shape, acc.shape)
        U = U + sk.double().abs()
    y, v = epilogue(acc, scale=scale, bias=bias, floor=floor, skip=sk, relu_pre=relu_pre, relu_post=relu_post)
    return Ref(y, v, U, K)


def conv3d(x, w, *, kind, transposed=False, K=0, **epi):
    """x [B,D,H,W,>=c_in] holding storage-type values (channels past c_in are not read), w fp32 [c_out,c_in,3,3,3] (or
    [c_in,c_out,3,3,3] with ``transposed``) holding storage-type values, scale / bias / floor [c_out], skip [B,Do,Ho,Wo,*] read at
    ``skip_coff``, relu_pre / relu_post -> Ref."""
    acc, Uacc = contract(x, w, kind=kind, transposed=transposed)
    return finish(acc, Uacc, K=K, **epi)


def acc_nonfinite(x, w, *, kind, transposed=False):
    """[B,Do,Ho,Wo] bool: output voxels whose receptive field holds a non-finite input value (every channel: 0 * NaN = NaN)."""
    wg = gather_weight(w, kind, transposed)
    bad = (~torch.isfinite(x[..., :wg.shape[1]].double())).double()
    return accumulate(bad, torch.ones_like(wg[:1]), kind)[..., 0] > 0


# ------------------------------------------------------------------------------------------------------------------------------
# The case table: one row per instantiation the host can select.
#   kernel   "brick" conv3d_kernel | "wide" conv3d_widep_kernel | "pair" conv3d_sweep8_kernel (plane pairs in the MFMA rows) |
#            "kdm" conv3d_sweep8_kdm_kernel (kd in the rows) | "narrow" conv3d_sweepc_kernel | "s2sweep" conv3d_sweep_s2_kernel |
#            "t2p8" conv3d_t2p8_kernel | "c1" conv3d_c1_kernel | "c1sweep" conv3d_c1_sweep_kernel
#   kind     "S1" | "S2" | "T2": what the layer computes (Conv3dLayer.build turns it into S1P8 / T2P8 / S1C1 where ``sweep`` says so)
#   knobs    pscv_set_tuning values that select the instantiation
#   sweep    (ops.USE_SWEEP_KERNEL, ops.SWEEP16) while the layer is built
#   cat2     the 16 input channels come from two tensors (pscv_conv3d_cat2)
#   twin     knobs of another instantiation that must give the same bits (None: no such claim), twin32: for fp32 outputs only
#   halo     depth planes (of the input grid) beyond ATen's footprint that a non-finite input voxel may turn into NaN: the kernel
#            multiplies it with zero-weight rows of its MFMA operand (0 x NaN = NaN)
#   sizes    [(D, H, W, size knobs)]; a size knob "s2s_chunks": n stands for s2s_slots = n x the launch's in-plane tiles
#   edge     the row also runs the epilogue-edge tests (one row per kernel, tile variant and store instance)
# ------------------------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "name kernel c_in c_out kind transposed knobs sweep cat2 twin twin32 halo sizes edge")
CASES = []
BRICK_LINES = [(8, 1), (8, 2), (16, 1), (16, 2), (32, 1), (32, 2), (32, 4), (64, 2), (64, 4)]      # PSCV_CONV_CASE(c_in, n_tiles)
ONE = (1, 1, 1, {})
# Sizes: the smallest with two tiles per axis whose last tile is one voxel thick (tile constants of the kernels, in comments).
BRICK_SIZES = {
    ("S1", 0): [ONE, (5, 5, 17, {})],            # launch_kind: 4 x 4 x 16 output voxels
    ("S1", 1): [ONE, (2, 5, 17, {})],            # small volumes: 1 x 4 x 16, the waves split the reduction (KSPLIT)
    ("S1", "tall"): [ONE, (5, 9, 17, {})],       # 4 x 8 x 16 (64 input channels)
    ("S2", 0): [ONE, (5, 5, 33, {})],            # 2 x 2 x 16 OUTPUT voxels: outputs 3 x 3 x 17
    ("T2", 0): [ONE, (3, 5, 17, {})],            # 2 x 4 x 16 INPUT voxels
    ("T2", 1): [ONE, (2, 5, 17, {})],            # small volumes: 1 x 4 x 16 input voxels, the waves split the parity classes (CSPLIT)
}
# Depth sweeps: sweep_dc = 16 at D = 17 makes one chunk of 16 planes (the 6-slot / 3-slot rings wrap more than twice) and one of a
# single plane; sweep_dc = 4 at D = 9 makes chunks of 4, 4 and 1 planes (a seam on both sides of a chunk).  8 x 16 pixel tiles
# (16 x 16 with sweep_th16, which the launcher takes from H = 16 on): H = 9 / 17, W = 17.
SWEEP_SIZES = [ONE, (17, 9, 17, {"sweep_dc": 16}), (9, 9, 17, {"sweep_dc": 4})]
SWEEP_SIZES_TH16 = [ONE, (17, 17, 17, {"sweep_dc": 16}), (9, 17, 17, {"sweep_dc": 4})]
# Stride-2 sweep: 8 x 16 output pixels, 5-slot ring, two slots per output plane; s2s_slots = tiles gives ONE chunk (11 output planes:
# the ring wraps four times), s2s_slots = 2 tiles at 5 output planes gives chunks of 4 and 1 (plan_depth_chunk: at least 4 planes).
S2S_SIZES = [ONE, (21, 17, 33, {"s2s_chunks": 1}), (9, 17, 33, {"s2s_chunks": 2})]
# 1-channel head: 4 x 32 pixels x 6-plane blocks.  Brick variant: c1_nb = 1 / 2 blocks per workgroup, the last block one plane thick.
# Sweep variant (16-slot ring): by default one block per chunk on a small volume (chunks of 6 and 1 planes at D = 7); c1_nb = 6 at
# D = 37 makes a chunk of 36 planes (the ring wraps twice) and one of a single plane.
C1_SIZES = [ONE, (7, 5, 33, {"c1_nb": 1}), (13, 5, 33, {"c1_nb": 2})]
C1S_SIZES = [ONE, (7, 5, 33, {}), (37, 5, 33, {"c1_nb": 6})]
T2P8_SIZES = [ONE, (3, 5, 17, {})]               # 2 x 4 x 16 input voxels


def _add(name, kernel, c_in, c_out, kind, knobs, sizes, *, transposed=False, sweep=(False, False), cat2=False, twin=None, twin32=False,
         halo=0, edge=False):
    CASES.append(Case(name, kernel, c_in, c_out, kind, transposed or kind == "T2", dict(knobs), sweep, cat2, twin, twin32, halo, sizes, edge))


def _brick_rows():
    off = {"conv_wide": 0, "conv_tall64": 0, "conv_s2_sweep": 0}
    for ci, nt in BRICK_LINES:
        co = 16 * nt
        nts = [n for n in (1, 2, 4) if n <= nt]
        # S1: the large tile, the small tile with every conv_small_nt that divides the tile count, the tall tile (c_in = 64)
        _add(f"brick{ci}to{co}S1", "brick", ci, co, "S1", dict(off, conv_small_tiles=0), BRICK_SIZES[("S1", 0)], edge=(ci, nt) == (16, 1))
        for n in nts:
            _add(f"brick{ci}to{co}S1small{n}", "brick", ci, co, "S1", dict(off, conv_small_tiles=1, conv_small_nt=n), BRICK_SIZES[("S1", 1)],
                 edge=(ci, nt, n) == (8, 2, 1))
        if ci == 64:
            _add(f"brick{ci}to{co}S1tall", "brick", ci, co, "S1", dict(off, conv_small_tiles=0, conv_tall64=2), BRICK_SIZES[("S1", "tall")],
                 twin=dict(off, conv_small_tiles=0))
        if nt == (2 if ci >= 32 else 1):         # a stride-1 ConvTranspose3d per c_in (the flipped kernel goes through the packing)
            _add(f"brick{ci}to{co}S1tr", "brick", ci, co, "S1", dict(off, conv_small_tiles=1, conv_small_nt=0), BRICK_SIZES[("S1", 1)], transposed=True)
        # S2: all tiles in one workgroup by default, the conv_small_nt overrides
        for n in ([0] if nt == 1 else nts):
            _add(f"brick{ci}to{co}S2nt{n}", "brick", ci, co, "S2", dict(off, conv_small_nt=n), BRICK_SIZES[("S2", 0)], edge=(ci, nt, n) == (16, 2, 2))
        # T2: as S1
        _add(f"brick{ci}to{co}T2", "brick", ci, co, "T2", dict(off, conv_small_tiles=0), BRICK_SIZES[("T2", 0)], edge=(ci, nt) == (32, 1))
        for n in nts:
            _add(f"brick{ci}to{co}T2small{n}", "brick", ci, co, "T2", dict(off, conv_small_tiles=1, conv_small_nt=n), BRICK_SIZES[("T2", 1)],
                 edge=(ci, nt, n) == (16, 1, 1))


_brick_rows()
for _ci, _co in ((64, 64), (64, 32), (32, 64), (32, 32)):
    _add(f"wide{_ci}to{_co}", "wide", _ci, _co, "S1", {"conv_wide": 2}, [ONE, (5, 5, 17, {})],
         twin={"conv_wide": 0, "conv_small_tiles": 0, "conv_tall64": 0}, edge=(_ci, _co) == (32, 32))
SW = (True, False)
for _th in (0, 1):
    _add(f"pair32to8th16_{_th}", "pair", 32, 8, "S1", {"sweep_th16": _th, "sweep_kdm": 0}, SWEEP_SIZES_TH16 if _th else SWEEP_SIZES, sweep=SW, halo=2, edge=True)
_add("pair32to8tr", "pair", 32, 8, "S1", {"sweep_th16": 0, "sweep_kdm": 0}, SWEEP_SIZES, sweep=SW, halo=2, transposed=True)
for _kdm in (1, 2):
    for _pd in (1, 2):
        _add(f"kdm{_kdm}pd{_pd}", "kdm", 32, 8, "S1", {"sweep_kdm": _kdm, "sweep_kdm_pd": _pd}, SWEEP_SIZES, sweep=SW, edge=(_kdm, _pd) == (1, 2))
for _ci, _co in ((8, 8), (16, 8), (16, 16)):
    _sw = (True, _co == 16)
    for _pd in (1, 2, 3):
        _add(f"narrow{_ci}to{_co}pd{_pd}", "narrow", _ci, _co, "S1", {"sweepc_pd": _pd}, SWEEP_SIZES, sweep=_sw, halo=0 if _co == 16 else 2,
             edge=_pd == 1 and _ci == _co)
    _add(f"narrow{_ci}to{_co}tr", "narrow", _ci, _co, "S1", {"sweepc_pd": 0}, SWEEP_SIZES, sweep=_sw, halo=0 if _co == 16 else 2, transposed=True)
for _co in (8, 16):
    _add(f"cat2to{_co}", "narrow", 16, _co, "S1", {"sweepc_pd": 0}, SWEEP_SIZES, sweep=(True, True), cat2=True, halo=0 if _co == 16 else 2)
for _co in (16, 24, 32):
    _add(f"s2sweep8to{_co}", "s2sweep", 8, _co, "S2", {"conv_s2_sweep": 2}, S2S_SIZES, edge=_co == 16)
_add("t2p8", "t2p8", 16, 8, "T2", {}, T2P8_SIZES, sweep=SW, edge=True)
# (a non-finite voxel of input plane d0 + 6 reaches output plane d0 of its 6-plane block through the zero entries of the banded
#  depth-in-rows operand: 6 planes in general, 3 for a voxel in planes 2 or 3 (mod 6) of a block, where the edge tests put theirs)
_add("c1in8", "c1", 8, 1, "S1", {"c1_sweep": 0}, C1_SIZES, sweep=SW, halo=6, edge=True)
_add("c1in8sweep", "c1sweep", 8, 1, "S1", {"c1_sweep": 2}, C1S_SIZES, sweep=SW, halo=6, twin={"c1_sweep": 0}, twin32=True, edge=True)
_add("c1in16", "c1", 16, 1, "S1", {"c1_sweep": 0}, C1_SIZES, sweep=SW, halo=6, edge=True)
_add("c1in16knob2", "c1", 16, 1, "S1", {"c1_sweep": 2}, C1_SIZES, sweep=SW, halo=6)      # (the sweep variant is for 8 input channels: same kernel)

BY_NAME = {c.name: c for c in CASES}
EDGE_CASES = [c for c in CASES if c.edge]
WIDE_CASES = [c for c in CASES if c.kernel == "wide"]
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}
EPILOGUES = ("bn_relu_skip", "bn_skip_relupost", "bias_only", "none")
HALO_MAX = 3        # the bar of tests/test_gpu_conv3d.py::test_conv3d_epilogue_propagates_nan_like_torch_relu, kept by the edge tests


def k_terms(c):
    """Product terms (zero-weight padding included) in the MFMA chains of one output element, from the kernels' code."""
    ci = c.c_in
    if c.kernel in ("brick", "s2sweep") and c.kind != "T2":
        return 32 * math.ceil(27 * ci / 32)   # conv_total_steps / S2S_STEPS: k = (tap, c_in) flattened, padded to 32-deep MFMA steps
    if c.kernel == "brick":
        return 32 * math.ceil(8 * ci / 32)    # T2: the parity class with all 8 taps has the longest chain (t2_nsteps(7, c_in))
    if c.kernel == "wide":
        return 27 * ci                        # NSTEPS = 27 c_in / 32 steps of 32, no padding (c_in 32 | 64)
    if c.kernel == "pair":
        return 4 * 9 * 32                     # 4 input planes x 9 taps x 32 channels per plane pair, one of the 4 planes with zero weights
    if c.kernel == "kdm":
        return 3 * 9 * 32                     # 3 iterations x 18 MFMAs of 16: an output's 8 rows see exactly its 3 planes
    if c.kernel == "narrow":
        return 4 * 9 * ci                     # NM = 36 c_in / 32 MFMAs per output: 4 planes (c_out 8) or 2 x 2 planes, one repeated with zero weights (16)
    if c.kernel == "t2p8":
        return 4 * 32                         # class (pd, ph) = (1, 1): 4 MFMAs of (2 w-taps x 16 channels)
    if c.kernel in ("c1", "c1sweep"):
        return 8 * 9 * ci                     # NSTEPS = 72 c_in / 32: 8 input planes x 9 taps per 6-plane block (banded weights)
    raise ValueError(c.kernel)


def batch_of(size_index):
    """B = 2 and B = 3 alternate over a row's sizes."""
    return 2 + size_index % 2


def epilogue_of(case_index, size_index):
    return EPILOGUES[(case_index + size_index) % 4]


def resolve_knobs(c, B, D, H, W, size_knobs):
    """The row's knobs and the size's, with the pseudo knob s2s_chunks turned into s2s_slots."""
    kn = dict(c.knobs)
    for k, v in size_knobs.items():
        if k == "s2s_chunks":
            _, Ho, Wo = out_dhw("S2", D, H, W)
            kn["s2s_slots"] = v * B * ((Ho + 7) // 8) * ((Wo + 15) // 16)
        else:
            kn[k] = v
    return kn


def depth_chunks(c, B, D, H, W, kn):
    """Planes (output planes for the stride-2 sweep) of each depth chunk the launchers make for these knobs at a SMALL volume (fewer
    tiles than resident slots), restated from plan_depth_chunk / c1_dispatch: the CPU file asserts the seams the sizes are meant for."""
    def cut(n, dc):
        return [min(dc, n - s) for s in range(0, n, dc)]
    if c.kernel in ("pair", "kdm", "narrow"):
        even = c.kernel != "kdm"
        th = 16 if (c.kernel == "pair" and kn.get("sweep_th16") and H >= 16) else 8
        tiles = B * ((H + th - 1) // th) * ((W + 15) // 16)
        slots = {"pair": 256 if th == 16 else 512, "kdm": 1024 if kn.get("sweep_kdm", 0) >= 2 else 768, "narrow": 512 if c.c_out == 16 else 768}[c.kernel]
        want = 1 if tiles >= slots else slots // tiles
        dc = -(-D // want)
        dc = (dc + 1) & ~1 if even else dc
        dc = max(dc, 4)
        f = kn.get("sweep_dc", 0)
        if f > 0:
            dc = f & ~1 if even else f
        dc = ((D + 1) & ~1 if even else D) if dc > D else dc
        return cut(D, dc)
    if c.kernel == "s2sweep":
        Do, Ho, Wo = out_dhw("S2", D, H, W)
        tiles = B * ((Ho + 7) // 8) * ((Wo + 15) // 16)
        slots = kn.get("s2s_slots", 0) or 768
        want = 1 if tiles >= slots else slots // tiles
        dc = max(-(-Do // want), 4)
        return cut(Do, min(dc, Do))
    if c.kernel == "c1sweep":
        tiles = B * ((H + 3) // 4) * ((W + 31) // 32)
        nblocks = (D + 5) // 6
        want = 1 if tiles >= 768 else 768 // tiles
        ndc = min(want, nblocks)
        nbk = -(-nblocks // ndc)
        if kn.get("c1_nb", 0) > 2:
            nbk = min(kn["c1_nb"], nblocks)
        return cut(D, 6 * nbk)
    if c.kernel == "c1":
        return cut(D, 6 * kn["c1_nb"]) if kn.get("c1_nb") else [D]
    return [D]


def long_volume(n_cu=256):
    """(B, D, H, W, grid, tiles) of the volume on which every persistent workgroup of conv3d_widep_kernel takes a second 4 x 4 x 16
    tile and some a third: tiles >= 2 grid + 3 with grid = n_cu & ~7 (widep_launch), ragged in all three axes (D = 13: 4 depth tiles,
    W = 33: 3), and at least 512 tiles, so that the default conv_wide = 1 takes the kernel for 64 input channels as well."""
    grid = n_cu & ~7 if n_cu >= 8 else n_cu
    H = 4 * max(math.ceil((2 * grid + 3) / 12), 43) + 1
    return 1, 13, H, 33, grid, 12 * ((H + 3) // 4)


def make_operands(c, dtype, B, D, H, W, *, epilogue="none", seed=0, with_skip=True):
    """CPU operands of one launch of row ``c``: x [B,D,H,W,c_in] in ``dtype``; w fp32 holding ``dtype`` values, [c_out,c_in,3,3,3] or
    -- transposed rows -- [c_in,c_out,3,3,3]; bn (gamma, beta, mean, var) or None, gamma in +-(0.5 .. 1.5); conv_bias or None;
    (scale, bias) fp32 as Conv3dLayer.build folds them; skip [B,Do,Ho,Wo,c_out] in ``dtype``; relu_pre / relu_post."""
    g = torch.Generator().manual_seed(1000003 * (CASES.index(c) + 1) + 7919 * D + 131 * H + 17 * W + seed)
    x = torch.randn(B, D, H, W, c.c_in, generator=g).to(dtype)
    shape = (c.c_in, c.c_out, 3, 3, 3) if c.transposed else (c.c_out, c.c_in, 3, 3, 3)
    w = (torch.randn(shape, generator=g) / (27 * c.c_in / (8 if c.kind == "T2" else 1)) ** 0.5).to(dtype).float()
    bn = conv_bias = scale = bias = None
    relu_pre = relu_post = False
    co = c.c_out
    if epilogue in ("bn_relu_skip", "bn_skip_relupost"):
        sign = torch.where(torch.rand(co, generator=g) < 0.5, -1.0, 1.0)
        bn = ((torch.rand(co, generator=g) + 0.5) * sign, torch.randn(co, generator=g) * 0.1, torch.randn(co, generator=g) * 0.1,
              torch.rand(co, generator=g) + 0.5)
        scale, bias = fold_bn(*bn)
        relu_pre, relu_post = epilogue == "bn_relu_skip", epilogue == "bn_skip_relupost"
    elif epilogue == "bias_only":
        conv_bias = torch.randn(co, generator=g) * 0.2
        bias = conv_bias.clone()
    else:
        assert epilogue == "none", epilogue
    skip = torch.randn((B,) + out_dhw(c.kind, D, H, W) + (co,), generator=g).to(dtype) if with_skip else None
    return dict(x=x, w=w, bn=bn, conv_bias=conv_bias, scale=scale, bias=bias, skip=skip, relu_pre=relu_pre, relu_post=relu_post, floor=None)


def reference(c, o, *, with_skip, floor=None, relu_pre=None, relu_post=None):
    """Ref of row ``c`` on the operands ``o`` (the epilogue switches of ``o`` unless given).  The contraction is kept in ``o`` for the
    next call with the same ``x`` tensor (the edge tests run many epilogues on one launch's operands)."""
    kept = o.get("_contract")
    if kept is None or kept[0] is not o["x"]:
        kept = o["_contract"] = (o["x"],) + contract(o["x"], o["w"], kind=c.kind, transposed=c.transposed)
    return finish(kept[1], kept[2], scale=o["scale"], bias=o["bias"], floor=floor, skip=o["skip"] if with_skip else None,
                  relu_pre=o["relu_pre"] if relu_pre is None else relu_pre, relu_post=o["relu_post"] if relu_post is None else relu_post,
                  K=k_terms(c))


CYCLED_FLOORS = (-0.5, 0.25, -INF, 0.0)


def cycled_floor(c_out):
    return torch.tensor([CYCLED_FLOORS[i % 4] for i in range(c_out)])


def edge_size(c):
    """The row's ragged two-tile size (its second one) and its knobs, B = 2: what the epilogue-edge tests run."""
    D, H, W, kn = c.sizes[1]
    return 2, D, H, W, kn


def nonfinite_voxels(c, D, H, W):
    """Two input voxels (b, d, h, w), in different batch items, for +inf and NaN.  The 1-channel head gets depth planes 2 and 3 of a
    6-plane block (its zero-weight rows then reach no further than HALO_MAX planes); deep volumes get the NaN in their last plane but
    one: beside the seam of the sizes' last, one-plane chunk."""
    d_inf = min(2, D // 2)
    d_nan = min(3, D // 2) if c.kernel in ("c1", "c1sweep") or D < 9 else D - 2
    return (0, d_inf, H // 3, W // 4), (1, d_nan, (2 * H) // 3, (3 * W) // 4)


def inf_may_turn_nan(c):
    """Kernels whose reduction meets a voxel of an output's own footprint a second time with a zero weight (0 x inf = NaN where ATen
    has +-inf): the k padding of conv3d_kernel and conv3d_sweep_s2_kernel re-reads the last tap's voxel where 27 c_in (T2: taps x
    c_in of a parity class) is no multiple of 32; the 16 -> 16 sweep reads the output's own plane twice.  The other kernels meet every
    (output, input voxel) pair once, with its weight or -- outside the footprint -- with a zero (``halo``)."""
    if c.kernel in ("brick", "s2sweep"):
        return c.c_in % 32 != 0
    return c.kernel == "narrow" and c.c_out == 16


def skip_voxels(c, shape):
    """Three output voxels (b, d, h, w) of a skip tensor [B,Do,Ho,Wo,*]: they get -inf, +inf and NaN in every channel."""
    B, Do, Ho, Wo = shape[:4]
    return (0, 0, Ho - 1, Wo // 2), (1, Do - 1, 0, Wo - 1), (B - 1, Do // 2, Ho // 2, 0)


def poison_skip_and_bias(c, o, vox):
    """-inf, +inf and NaN at the three skip voxels; -inf as the bias of the last output channel (layers with more than one)."""
    nan = float("nan")
    o["skip"][vox[0]], o["skip"][vox[1]], o["skip"][vox[2]] = -INF, INF, nan
    if c.c_out > 1:
        bias = torch.zeros(c.c_out) if o["bias"] is None else o["bias"].clone()
        bias[c.c_out - 1] = -INF
        o["bias"] = bias
