"""Tensor-level host wrappers over the pscv C ABI (include/pscv.h).

PyTorch is plumbing here: it owns device memory and the stream; every op below hands raw device
pointers to ``libpscv.so`` on ``torch.cuda.current_stream()``.  Nothing in this module computes the
hot path with torch ops, and every entry point raises if the tensors are not on a HIP device.

Layouts: feature maps ``[B,h,w,C]`` and volumes ``[B,D,h,w,C]`` (channels-last), bf16 or fp32 storage.
"""
from __future__ import annotations

import collections
import ctypes as C
import functools
import math
import weakref
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib as L

_TORCH2PSCV = {torch.float32: L.F32, torch.bfloat16: L.BF16, torch.float16: L.F16}
HALF_DTYPES = (torch.bfloat16, torch.float16)


def _dt(t: torch.Tensor) -> int:
    try:
        return _TORCH2PSCV[t.dtype]
    except KeyError:
        raise TypeError(f"pscv: unsupported dtype {t.dtype} (float32 / bfloat16 / float16 only)")


def _dev(*ts: Optional[torch.Tensor]):
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError("pscv: the plane-sweep engine runs on MI355X only; got a CPU tensor "
                               "(there is no CPU / PyTorch fallback for the hot path)")
        if not t.is_contiguous():
            raise ValueError("pscv: tensors handed to the C ABI must be contiguous")


def _p(t: Optional[torch.Tensor]):
    """Device address for a ``c_void_p`` parameter (every entry point declares its argtypes): the plain integer / None -- ctypes
    converts it at the call; building a ``c_void_p`` object per pointer cost ~2 us per launch."""
    return None if t is None else t.data_ptr()


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_cur_device = getattr(torch._C, "_cuda_getDevice", None)


def _stream():
    """Raw handle of the current HIP stream.  ``torch.cuda.current_stream()`` builds a Stream object through several Python layers
    (~4-7 us per call -- more than the ctypes launch itself, and a forward of Vis-MVSNet makes ~300 launches); the C-level accessor
    is the same query without the object."""
    if _raw_stream is not None and _cur_device is not None:
        return _raw_stream(_cur_device())
    return torch.cuda.current_stream().cuda_stream


class EventTimer:
    """Per-kernel HIP-event timing on the launch stream (used by bench.py for the roofline figures).

    ``with EventTimer() as tm: ...`` brackets every pscv launch with a pair of events recorded on the
    stream the kernel is launched on; ``tm.summary()`` (after a device sync) returns
    ``{name: (launches, total_ms)}``."""

    def __init__(self):
        self.records = []
        self.costs = []

    def __enter__(self):
        global _timer
        self._prev, _timer = _timer, self
        return self

    def __exit__(self, *exc):
        global _timer
        _timer = self._prev
        return False

    def launch(self, name, fn, cost=None):
        st = torch.cuda.current_stream()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        rc = fn()
        e1.record(st)
        self.records.append((name, e0, e1))
        if cost is not None:
            self.costs.append((name,) + tuple(cost()))
        return rc

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for name, e0, e1 in self.records:
            n, ms = out.get(name, (0, 0.0))
            out[name] = (n + 1, ms + e0.elapsed_time(e1))
        return out

    def detail(self):
        """{name: dict(launches, ms, bytes, flops)}: ``bytes`` / ``flops`` are the ALGORITHMIC HBM bytes (operands read once,
        results written once) and floating-point operations the launches of that name asked for (conv3d / conv2d / warp_cost
        report them; 0 for the others)."""
        out = {k: dict(launches=n, ms=ms, bytes=0.0, flops=0.0) for k, (n, ms) in self.summary().items()}
        for name, b, f in self.costs:
            out[name]["bytes"] += b
            out[name]["flops"] += f
        return out


_timer: Optional[EventTimer] = None


def _launch(name, fn, cost=None):
    """Run a C-ABI launch; under an EventTimer it is bracketed by HIP events and ``cost()`` -> (algorithmic bytes, flops) is
    recorded with it (evaluated only then)."""
    return _timer.launch(name, fn, cost) if _timer is not None else fn()


# --------------------------------------------------------------------------------------------
# layout helpers (plumbing)
# --------------------------------------------------------------------------------------------
def to_channels_last(x: torch.Tensor, dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    """[B,C,h,w] -> [B,h,w,C] or [B,C,D,h,w] -> [B,D,h,w,C], contiguous, in the storage dtype."""
    perm = (0, 2, 3, 1) if x.dim() == 4 else (0, 2, 3, 4, 1)
    return x.permute(*perm).to(dtype).contiguous()


def to_channels_first(x: torch.Tensor) -> torch.Tensor:
    """View a channels-last pscv tensor with the reference's NCHW / NCDHW index order (no copy)."""
    perm = (0, 3, 1, 2) if x.dim() == 4 else (0, 4, 1, 2, 3)
    return x.permute(*perm)


# --------------------------------------------------------------------------------------------
# cameras (A0; stays torch, fp64 closed forms, no LAPACK call on the device)
# --------------------------------------------------------------------------------------------
def inv3x3(m: torch.Tensor) -> torch.Tensor:
    """Batched adjugate inverse of [...,3,3]."""
    a, b, c = m[..., 0, 0], m[..., 0, 1], m[..., 0, 2]
    d, e, f = m[..., 1, 0], m[..., 1, 1], m[..., 1, 2]
    g, h, i = m[..., 2, 0], m[..., 2, 1], m[..., 2, 2]
    co = torch.stack([e * i - f * h, c * h - b * i, b * f - c * e,
                      f * g - d * i, a * i - c * g, c * d - a * f,
                      d * h - e * g, b * g - a * h, a * e - b * d], dim=-1)
    det = a * co[..., 0] + b * co[..., 3] + c * co[..., 6]
    return (co / det.unsqueeze(-1)).reshape(m.shape)


def proj_cams(src_projs: Sequence[torch.Tensor], ref_proj: torch.Tensor) -> torch.Tensor:
    """PROJ-geometry camera block [n_src,B,18]: rot[9], trans[3] of ``P_src P_ref^-1``
    (reference models/MVSNet/module.py:128-130).  Projection matrices are [B,4,4] with last row (0,0,0,1)."""
    Pr = ref_proj.double()
    Ar_inv = inv3x3(Pr[:, :3, :3])
    br = Pr[:, :3, 3:4]
    out = []
    for Ps in src_projs:
        Ps = Ps.double()
        rot = Ps[:, :3, :3] @ Ar_inv
        trans = Ps[:, :3, 3:4] - rot @ br
        blk = torch.cat([rot.reshape(-1, 9), trans.reshape(-1, 3), torch.zeros_like(rot.reshape(-1, 9)[:, :6])], dim=1)
        out.append(blk)
    return torch.stack(out).to(torch.float32).contiguous()


def proj_cams_device(proj: torch.Tensor, reference_frame: int = 0) -> torch.Tensor:
    """Same block as ``proj_cams`` for all source views of ``proj`` [B,V,4,4] in ONE HIP launch
    (pscv_proj_cams): [V-1,B,18], sources in view order with the reference skipped."""
    _dev(proj)
    if proj.dim() != 4 or proj.shape[2:] != (4, 4) or proj.dtype != torch.float32:
        raise ValueError("pscv.proj_cams_device: proj must be fp32 [B,V,4,4]")
    B, V = proj.shape[:2]
    cams = torch.empty((V - 1, B, L.CAM_FLOATS), dtype=torch.float32, device=proj.device)
    rc = _launch("proj_cams", lambda: L.lib().pscv_proj_cams(_p(proj), B, V, int(reference_frame), _p(cams), _stream()))
    L.check(rc, "pscv_proj_cams")
    return cams


def batch_views(ts: Sequence[torch.Tensor]) -> torch.Tensor:
    """``torch.cat(ts, 0)`` -- as a VIEW when the tensors are back-to-back slices of one buffer (the views of an image batch
    [1,V,3,H,W] picked with ``imgs[:, i]``): the extractors batch all views without a copy."""
    v = _consecutive_views(ts)
    if v is None:
        return torch.cat(list(ts), 0)
    return v.reshape((len(ts) * ts[0].shape[0],) + tuple(ts[0].shape[1:]))


def _consecutive_views(ts: Sequence[torch.Tensor]) -> Optional[torch.Tensor]:
    """[n, *shape] view over ``ts`` when they are equally shaped contiguous tensors lying back to back in one storage (e.g.
    ``base[1:].unbind(0)``): no copy.  None otherwise."""
    ts = list(ts)
    t0 = ts[0]
    if not all(t.is_contiguous() and t.shape == t0.shape and t.dtype == t0.dtype and t.device == t0.device
               and t.untyped_storage().data_ptr() == t0.untyped_storage().data_ptr() for t in ts):
        return None
    step = t0.numel()
    if step == 0 or any(t.storage_offset() != t0.storage_offset() + i * step for i, t in enumerate(ts)):
        return None
    return torch.as_strided(t0, (len(ts),) + tuple(t0.shape), (step,) + tuple(t0.stride()))


def homog_cams_device(ref_cam: torch.Tensor, src_cams: Sequence[torch.Tensor], scale: float) -> torch.Tensor:
    """HOMOG-geometry camera blocks [n_src,B,18] (A[9], Bm[9]) from Vis-style cam arrays [B,2,4,4] in one HIP
    launch (pscv_homog_cams); ``scale`` = 1 / s_scale is applied to the intrinsics like scale_camera."""
    src = _consecutive_views(src_cams)
    if src is None:
        src = torch.stack(list(src_cams))
    src = src.to(torch.float32).contiguous()
    ref = ref_cam.to(torch.float32).contiguous()
    _dev(ref, src)
    n, B = src.shape[:2]
    cams = torch.empty((n, B, L.CAM_FLOATS), dtype=torch.float32, device=ref.device)
    rc = _launch("homog_cams", lambda: L.lib().pscv_homog_cams(_p(ref), _p(src), B, n, float(scale), _p(cams), _stream()))
    L.check(rc, "pscv_homog_cams")
    return cams


def fuse_pairs(interms: Sequence[torch.Tensor], uncerts: Sequence[torch.Tensor], *, normalise: bool = True,
               want_wsum: bool = False):
    """interms n x [B,D,h,w,8] (16-bit), uncerts n x [B,h,w] fp32 -> fused [B,D,h,w,8] (same dtype, normalised)
    or fp32 partial sums (normalise=False); optionally also the weight sum [B,h,w]."""
    interms, uncerts = list(interms), list(uncerts)
    _dev(*interms, *uncerts)
    B, D, h, w, c = interms[0].shape
    if c != 8 or any(t.shape != interms[0].shape or t.dtype != interms[0].dtype for t in interms):
        raise ValueError("pscv.fuse_pairs: pair volumes must share shape [B,D,h,w,8] and dtype")
    if any(u.dtype != torch.float32 or tuple(u.shape) != (B, h, w) for u in uncerts) or len(uncerts) != len(interms):
        raise ValueError("pscv.fuse_pairs: uncertainty maps must be fp32 [B,h,w], one per pair volume")
    n = len(interms)
    out = torch.empty((B, D, h, w, 8), dtype=interms[0].dtype if normalise else torch.float32, device=interms[0].device)
    wsum = torch.empty((B, h, w), dtype=torch.float32, device=out.device) if want_wsum else None
    ip = (C.c_void_p * n)(*[t.data_ptr() for t in interms])
    up = (C.c_void_p * n)(*[t.data_ptr() for t in uncerts])
    rc = _launch("fuse_pairs", lambda: L.lib().pscv_fuse_pairs(ip, up, n, _dt(interms[0]), _p(out), _p(wsum), int(normalise),
                                                               B, D, h, w, _stream()))
    L.check(rc, "pscv_fuse_pairs")
    return (out, wsum) if want_wsum else out


def fuse_finish(partial: torch.Tensor, wsum: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """partial fp32 [B,D,h,w,8] (all-reduced sum of w*interm), wsum fp32 [B,h,w] -> normalised 16-bit volume."""
    _dev(partial, wsum)
    B, D, h, w, c = partial.shape
    if c != 8 or partial.dtype != torch.float32 or tuple(wsum.shape) != (B, h, w) or wsum.dtype != torch.float32:
        raise ValueError("pscv.fuse_finish: partial fp32 [B,D,h,w,8] and wsum fp32 [B,h,w] expected")
    out = torch.empty((B, D, h, w, 8), dtype=dtype, device=partial.device)
    rc = _launch("fuse_finish", lambda: L.lib().pscv_fuse_finish(_p(partial), _p(wsum), _TORCH2PSCV[dtype], _p(out), B, D, h, w, _stream()))
    L.check(rc, "pscv_fuse_finish")
    return out


# --------------------------------------------------------------------------------------------
# 2-D feature extractor layers (the step before the path)
# --------------------------------------------------------------------------------------------
def pack_conv2d_weights(weight: torch.Tensor, c_in_padded: int, dtype: torch.dtype = torch.float16) -> np.ndarray:
    """Host-side repack of a Conv2d weight [Co,Ci,k,k] (k = 3 or 5) into the MFMA fragment order of pscv_conv2d for
    an input that carries ``c_in_padded`` >= Ci channels (uint16 bit patterns of ``dtype``)."""
    w = np.ascontiguousarray(weight.detach().to("cpu", torch.float32).numpy())
    if w.ndim != 4 or w.shape[2] != w.shape[3]:
        raise ValueError(f"pscv: conv2d weights must be [Co,Ci,k,k], got {w.shape}")
    c_out, c_in, ks = w.shape[0], w.shape[1], w.shape[2]
    lib = L.lib()
    code = _TORCH2PSCV.get(dtype, -1)
    n = lib.pscv_pack_conv2d_weights(None, c_in, c_in_padded, c_out, ks, code, None)
    if n < 0:
        L.check(int(n), "pscv_pack_conv2d_weights")
    packed = np.empty(n, dtype=np.uint16)
    n2 = lib.pscv_pack_conv2d_weights(w.ctypes.data_as(C.c_void_p), c_in, c_in_padded, c_out, ks, code, packed.ctypes.data_as(C.c_void_p))
    if n2 != n:
        L.check(-1 if n2 >= 0 else int(n2), "pscv_pack_conv2d_weights")
    return packed


@dataclass
class Conv2dLayer:
    """One 2-D layer ready for the engine: packed 16-bit weights + fp32 epilogue vectors, on device."""
    packed: torch.Tensor
    dtype: torch.dtype
    c_in: int        # channels of the input map (padded count)
    c_out: int
    ks: int
    stride: int
    neg_slope: float   # activation max(v, neg_slope * v): 0 = ReLU, 0.1 = LeakyReLU(0.1), 1 = none
    scale: Optional[torch.Tensor] = None
    bias: Optional[torch.Tensor] = None

    @staticmethod
    def build(weight: torch.Tensor, *, stride: int, device=None, bn: Optional[Sequence[torch.Tensor]] = None,
              bn_eps: float = 1e-5, conv_bias: Optional[torch.Tensor] = None, relu: bool = False,
              leaky: Optional[float] = None, dtype: torch.dtype = torch.float16, adjoint: bool = False) -> "Conv2dLayer":
        """``bn`` = (gamma, beta, running_mean, running_var) folds an eval-mode BatchNorm2d into the epilogue;
        ``relu`` / ``leaky`` (negative slope) select the fused activation.  ``adjoint``: ``weight`` is a stride-1 FORWARD layer's
        [Co,Ci,k,k] and the result is its adjoint (Co -> Ci, taps flipped), packed straight from that tensor on the device."""
        device = device if device is not None else weight.device
        if adjoint:
            if not (weight.is_cuda and torch.device(device) == weight.device):
                return Conv2dLayer.build(weight.detach().float().flip(2, 3).transpose(0, 1).contiguous(), stride=stride, device=device, bn=bn,
                                         bn_eps=bn_eps, conv_bias=conv_bias, relu=relu, leaky=leaky, dtype=dtype)
            c_in, c_out, ks = int(weight.shape[0]), int(weight.shape[1]), int(weight.shape[2])
        else:
            c_out, c_in, ks = int(weight.shape[0]), int(weight.shape[1]), int(weight.shape[2])
        c_pad = (c_in + 7) // 8 * 8
        if weight.is_cuda and torch.device(device) == weight.device and weight.dim() == 4 and weight.shape[2] == weight.shape[3]:
            # device-side packing (same bits): no device -> host copy, no stream synchronisation per layer
            wd = weight.detach().to(torch.float32).contiguous()
            n = L.lib().pscv_pack_conv2d_weights(None, c_in, c_pad, c_out, ks, _TORCH2PSCV.get(dtype, -1), None)
            if n < 0:
                L.check(int(n), "pscv_pack_conv2d_weights")
            packed = torch.empty(int(n), dtype=torch.int16, device=weight.device)
            with torch.cuda.device(weight.device):
                L.check(L.lib().pscv_pack_conv2d_weights_device_ex(_p(wd), c_in, c_pad, c_out, ks, _TORCH2PSCV[dtype], int(adjoint), _p(packed),
                                                                   _stream()), "pscv_pack_conv2d_weights_device")
        else:
            packed = torch.from_numpy(pack_conv2d_weights(weight, c_pad, dtype).view(np.int16)).to(device)
        scale = bias = None
        if bn is not None:
            gamma, beta, mean, var = [t.detach().to(device, torch.float32) for t in bn]
            scale = gamma / torch.sqrt(var + bn_eps)
            bias = beta - mean * scale
            if conv_bias is not None:
                bias = bias + scale * conv_bias.detach().to(device, torch.float32)
            scale, bias = scale.contiguous(), bias.contiguous()
        elif conv_bias is not None:
            bias = conv_bias.detach().to(device, torch.float32).contiguous()
        slope = float(leaky) if leaky is not None else (0.0 if relu else 1.0)
        return Conv2dLayer(packed, dtype, c_pad, c_out, ks, int(stride), slope, scale, bias)


def conv2d_out_hw(layer: "Conv2dLayer", H: int, W: int, parity: int = -1):
    if layer.ks == 2 or parity >= 0:       # parity sub-convolution of a stride-2 transposed conv: full output map is 2x
        return 2 * H, 2 * W
    pad = layer.ks // 2
    return (H + 2 * pad - layer.ks) // layer.stride + 1, (W + 2 * pad - layer.ks) // layer.stride + 1


def conv2d(x: torch.Tensor, layer: Conv2dLayer, *, out_dtype: Optional[torch.dtype] = None, skip: Optional[torch.Tensor] = None,
           skip_coff: int = 0, out: Optional[torch.Tensor] = None, out_coff: int = 0, parity: int = -1) -> torch.Tensor:
    """x [B,H,W,C] in the layer's 16-bit format -> [B,Ho,Wo,c_out] in the same format or fp32 (pscv_conv2d_ex).
    ``skip`` is added before the activation; ``out`` / ``out_coff`` write a channel slice of a wider map; ``parity``
    (0..3) selects the output parity of a ks = 2 sub-convolution of a transposed conv (writes pixels (2i+py, 2j+px))."""
    _dev(x, layer.packed, skip, out)
    if x.dtype != layer.dtype or x.dim() != 4 or x.shape[3] != layer.c_in:
        raise TypeError(f"pscv.conv2d: input must be a {layer.dtype} [B,H,W,{layer.c_in}] map, got {x.dtype} {tuple(x.shape)}")
    out_dtype = layer.dtype if out_dtype is None else out_dtype
    B, H, W, _ = x.shape
    Ho, Wo = conv2d_out_hw(layer, H, W, parity)
    if out is None:
        out = torch.empty((B, Ho, Wo, layer.c_out), dtype=out_dtype, device=x.device)
    if tuple(out.shape[:3]) != (B, Ho, Wo):
        raise ValueError(f"pscv.conv2d: out has shape {tuple(out.shape)}, expected [B,{Ho},{Wo},*]")
    if skip is not None and (skip.dtype != layer.dtype or tuple(skip.shape[:3]) != (B, Ho, Wo)):
        raise ValueError("pscv.conv2d: skip must have the layer's dtype and the output's spatial shape")
    rc = _launch(f"conv2d[{layer.c_in}->{layer.c_out},k{layer.ks}s{layer.stride}]", lambda: L.lib().pscv_conv2d_ex(
        _p(x), _dt(x), _p(layer.packed), _p(layer.scale), _p(layer.bias), _p(skip), 0 if skip is None else skip.shape[3], skip_coff,
        _p(out), out.shape[3], out_coff, _dt(out), B, H, W, layer.c_in, layer.c_out, layer.ks, layer.stride, int(parity),
        float(layer.neg_slope), _stream()),
        # a parity launch (one of the four k2 sub-convolutions of a stride-2 transposed conv) writes ONE output pixel per input pixel --
        # a quarter of the 2H x 2W map it addresses -- so its output-side bytes and FLOPs count B*H*W pixels, not B*Ho*Wo
        cost=lambda: _conv_cost(B * H * W, B * H * W if parity >= 0 else B * Ho * Wo, layer.c_in, layer.c_out, layer.ks * layer.ks, False,
                                out.element_size(), skip is not None))
    L.check(rc, "pscv_conv2d")
    return out


_PARITY_K = {}


def deconv2d_parity_weights(weight: torch.Tensor):
    """ConvTranspose2d(k3, s2, p1, op1) weight [Ci,Co,3,3] -> four Conv2d weights [Co,Ci,2,2], index 2*py+px: output pixel
    (2i+py, 2j+px) = sum over taps (ty, tx) of W[py,px][:, :, ty, tx] x[i+ty, j+tx].  Along a dim, parity 0 takes input i with
    kernel index 1; parity 1 takes input i with kernel index 2 and input i+1 with kernel index 0."""
    w = weight.detach().float()
    ci, co = w.shape[:2]
    # kernel index per (parity, tap): parity 0 -> (1, none), parity 1 -> (2, 0); "none" reads a zero plane appended at index 3.
    # One indexed gather for all four sub-weights (16 slice assignments before: a training step rebuilds these per layer)
    wp = torch.nn.functional.pad(w, (0, 1, 0, 1))                                   # [ci,co,4,4], row / column 3 = zeros
    k = _PARITY_K.get(w.device)
    if k is None:
        k = _PARITY_K[w.device] = torch.tensor([[1, 3], [2, 0]], dtype=torch.long, device=w.device)
    W = wp[:, :, k[:, :, None, None], k[None, None, :, :]]                          # [ci,co,py,ty,px,tx]
    return [W[:, :, py, :, px, :].transpose(0, 1).contiguous() for py in (0, 1) for px in (0, 1)]


def image_to_channels_last8(x: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """[B,3,H,W] image -> [B,H,W,8] in the storage dtype, channels 3-7 zero (the first layer's padded input): one HIP launch
    (pscv_image_prep) for fp32 images on the GPU, torch ops otherwise."""
    B, c, H, W = x.shape
    if x.is_cuda and x.dtype == torch.float32 and c <= 8 and B <= 65535:
        x = x.contiguous()
        out = torch.empty((B, H, W, 8), dtype=dtype, device=x.device)
        rc = _launch("image_prep", lambda: L.lib().pscv_image_prep(_p(x), B, c, H, W, _dt(out), _p(out), None, None, _stream()))
        L.check(rc, "pscv_image_prep")
        return out
    out = torch.zeros((B, H, W, 8), dtype=dtype, device=x.device)
    out[..., :c] = x.permute(0, 2, 3, 1)
    return out


def image_pyramid_cl8(x: torch.Tensor, scales: int, dtype: torch.dtype) -> List[torch.Tensor]:
    """CVP's image pyramid in the extractor layout, finest first: level l+1 = F.interpolate(level l, scale_factor=0.5,
    mode='bilinear') (net.py:34-47), every level as [B,H_l,W_l,8] 16-bit pixels.  One launch per level reads the fp32 image once
    and writes its half-resolution fp32 image and that one's 8-channel form (pscv_image_prep); odd widths fall back to
    F.interpolate for that step."""
    B, c, H, W = x.shape
    if not (x.is_cuda and x.dtype == torch.float32 and c <= 8 and B <= 65535):
        raise TypeError("pscv.image_pyramid_cl8: fp32 [B,C<=8,H,W] images on the GPU expected")
    x = x.contiguous()
    levels = [image_to_channels_last8(x, dtype)]
    for l in range(1, scales):
        B, c, H, W = x.shape
        if W % 2 or H < 2:
            x = torch.nn.functional.interpolate(x, scale_factor=0.5, mode="bilinear", align_corners=None)
            levels.append(image_to_channels_last8(x, dtype))
            continue
        last = l == scales - 1
        half = None if last else torch.empty((B, c, H // 2, W // 2), dtype=torch.float32, device=x.device)
        cl = torch.empty((B, H // 2, W // 2, 8), dtype=dtype, device=x.device)
        rc = _launch("image_prep", lambda: L.lib().pscv_image_prep(_p(x), B, c, H, W, _dt(cl), None, _p(half), _p(cl), _stream()))
        L.check(rc, "pscv_image_prep")
        levels.append(cl)
        x = half
    return levels


# --------------------------------------------------------------------------------------------
# geometric-consistency filter (the step after the path)
# --------------------------------------------------------------------------------------------
def geo_filter_cams(K: torch.Tensor, R: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
    """[V,3,3], [V,3,3], [V,3,1] (view 0 = reference) -> camera blocks [V,30] fp32 (K, K^-1, R, t) for
    ``geo_filter``.  The inverse is ``torch.inverse`` in fp32, what the reference uses (utils_3D.py:131,155)."""
    K = K.to(torch.float32)
    blocks = torch.cat((K.reshape(-1, 9), torch.inverse(K).reshape(-1, 9), R.to(torch.float32).reshape(-1, 9),
                        t.to(torch.float32).reshape(-1, 3)), dim=1)
    return blocks.contiguous()


def _ptrs(tensors):
    """c_void_p array of the addresses of a list of tensors (a per-view pointer table of the C ABI)."""
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _hw(maps):
    """c_int array of the (h, w) pairs of a list of [h,w] maps."""
    return (C.c_int * (2 * len(maps)))(*[v for m in maps for v in m.shape])


def _maps(maps, what):
    """fp32 [h,w] device maps -> (the list, c_void_p array of their addresses, c_int array of their (h, w) pairs)."""
    maps = list(maps)
    _dev(*maps)
    for m in maps:
        if m.dtype != torch.float32 or m.dim() != 2:
            raise ValueError(f"{what}: fp32 [h,w] maps expected, got {m.dtype} {tuple(m.shape)}")
    return maps, _ptrs(maps), _hw(maps)


def _check_cams(cams, rows, what):
    """cams: fp32 camera blocks [rows, GEO_CAM_FLOATS] (``geo_filter_cams``); rows None accepts any number."""
    if cams.dtype != torch.float32 or cams.dim() != 2 or cams.shape[1] != L.GEO_CAM_FLOATS or (rows is not None and cams.shape[0] != rows):
        raise ValueError(f"{what}: fp32 cams [{'V' if rows is None else rows},{L.GEO_CAM_FLOATS}] expected (geo_filter_cams), "
                         f"got {cams.dtype} {tuple(cams.shape)}")


def _view_maps(what, depths, cams, *, lo, hi=None, cast):
    """Checked (depths, cams): ``cast`` makes them fp32 (geo_filter, fuse_depth_*, colmap_fuse*, view_covisibility, depth_normals), else
    only fp32 passes (the three tsdf_* operators).  The device is not looked at (``_one_device``)."""
    depths = list(depths)
    n = len(depths)
    if n < lo or (hi is not None and n > hi):
        raise ValueError(f"{what}: {f'{lo}..{hi} depth maps' if hi else 'at least one depth map'} expected, got {n}")
    if not torch.is_tensor(cams):
        raise ValueError(f"{what}: cams must be a tensor [V,{L.GEO_CAM_FLOATS}]")
    if cast:
        cams = cams.to(torch.float32)
    for v, d in enumerate(depths):
        if not (isinstance(d, torch.Tensor) and d.dim() == 2 and (cast or d.dtype == torch.float32)):
            raise ValueError(f"{what}: depth map {v} must be fp32 [h,w], got {getattr(d, 'dtype', type(d))} {tuple(getattr(d, 'shape', ()))}")
        depths[v] = (d if d.dtype == torch.float32 else d.to(torch.float32)).contiguous()
    _check_cams(cams, n or None, what)
    return depths, cams.contiguous()


def _view_colors(what, depths, colors):
    """One colour image per depth map, uint8 [h,w,3] or packed int32 [h,w] (``pack_rgba8``) -> the packed list."""
    colors = list(colors)
    if len(colors) != len(depths):
        raise ValueError(f"{what}: {len(depths)} depth maps and as many colour images expected, got {len(colors)}")
    packed = []
    for v, (d, c) in enumerate(zip(depths, colors)):
        if torch.is_tensor(c) and c.dtype == torch.int32 and tuple(c.shape) == tuple(d.shape):
            packed.append(c.contiguous())
        elif torch.is_tensor(c) and c.dtype == torch.uint8 and tuple(c.shape) == tuple(d.shape) + (3,):
            packed.append(pack_rgba8(c))
        else:
            raise ValueError(f"{what}: colours of view {v} must be uint8 [h,w,3] (or packed int32 [h,w]) at the depth map's size")
    return packed


def _one_device(what, names, *tensors):
    """Every tensor on the GPU, contiguous, and on the same one -> that device.  ``names`` says what they are in the message."""
    _dev(*tensors)
    dev = tensors[0].device
    if any(t.device != dev for t in tensors):
        raise ValueError(f"{what}: {names} must be on the same device")
    return dev


def _view_chunks(depths, cams):
    """The views in launches of at most FUSE_MAX_VIEWS: (slice, view count, depth pointers, (h, w) pairs, camera rows) of each."""
    for first in range(0, len(depths), L.FUSE_MAX_VIEWS):
        part = slice(first, min(first + L.FUSE_MAX_VIEWS, len(depths)))
        yield part, part.stop - first, _ptrs(depths[part]), _hw(depths[part]), cams[part]


def geo_filter(depth: torch.Tensor, src_depth: Sequence[torch.Tensor], cams: torch.Tensor, *, max_reproj_error: float = 1.0,
               depth_threshold: float = 0.01, min_tri_angle: float = 1.0, num_consistent: int = 3,
               want_counts: bool = False):
    """depth [h,w] fp32, src_depth N x [h_i,w_i] fp32, cams [N+1,30] (``geo_filter_cams``), all on the GPU ->
    (mask_depth, mask_disp, geo_mask) bool [h,w] (and int32 counts [3,h,w] with ``want_counts``): the masks of
    evaluation/filtering.py:73-83 in one launch (pscv_geo_filter)."""
    src_depth = list(src_depth)
    n = len(src_depth)
    if n < 1 or n > L.GEO_MAX_SRC:
        raise ValueError(f"pscv.geo_filter: depth [h,w] and 1..{L.GEO_MAX_SRC} source maps expected")
    (depth, *src_depth), cams = _view_maps("pscv.geo_filter", [depth] + src_depth, cams, lo=0, cast=True)
    _one_device("pscv.geo_filter", "depth maps and cams", cams, depth, *src_depth)
    ptrs, hw = _ptrs(src_depth), _hw(src_depth)
    h, w = depth.shape
    masks = torch.empty((3, h, w), dtype=torch.uint8, device=depth.device)
    counts = torch.empty((3, h, w), dtype=torch.int32, device=depth.device) if want_counts else None
    rc = _launch("geo_filter", lambda: L.lib().pscv_geo_filter(
        _p(depth), ptrs, hw, n, _p(cams), h, w, float(max_reproj_error), float(depth_threshold), float(min_tri_angle),
        int(num_consistent), _p(masks[0]), _p(masks[1]), _p(masks[2]), _p(counts), _stream()))
    L.check(rc, "pscv_geo_filter")
    out = (masks[0].bool(), masks[1].bool(), masks[2].bool())
    return out + (counts,) if want_counts else out


# --------------------------------------------------------------------------------------------
# depth-map fusion into a point cloud (the step after the geometric filter)
# --------------------------------------------------------------------------------------------
def pack_rgba8(colors: torch.Tensor) -> torch.Tensor:
    """uint8 [h,w,3] -> int32 [h,w] with the bytes R, G, B, 0 (red in the low byte): one 32-bit gather per colour (layout only)."""
    if colors.dtype != torch.uint8 or colors.dim() != 3 or colors.shape[2] != 3:
        raise ValueError("pscv.pack_rgba8: uint8 [h,w,3] colours expected")
    pad = torch.zeros(colors.shape[:2] + (1,), dtype=torch.uint8, device=colors.device)
    return torch.cat((colors, pad), dim=2).contiguous().view(torch.int32).reshape(colors.shape[:2])


def _fuse_inputs(depths, colors, cams):
    what = "pscv.fuse_depth"
    depths, cams = _view_maps(what, depths, cams, lo=2, hi=L.FUSE_MAX_VIEWS, cast=True)
    packed = _view_colors(what, depths, colors)
    dev = _one_device(what, "depth maps, colours and cams", cams, *depths, *packed)
    ws_bytes = max(int(L.lib().pscv_fuse_depth_workspace(int(d.shape[0]), int(d.shape[1]))) for d in depths)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    return depths, packed, cams, (_ptrs(depths), _ptrs(packed), _hw(depths)), ws


def _check_used(used, depths):
    if len(used) != len(depths):
        raise ValueError("pscv.fuse_depth: one used mask per view expected")
    for v, (u, d) in enumerate(zip(used, depths)):
        _dev(u)
        if u.dtype != torch.uint8 or tuple(u.shape) != tuple(d.shape):
            raise ValueError(f"pscv.fuse_depth: used mask {v} must be uint8 [h,w] at the depth map's size")


def _fuse_pass(i, depths, ptrs, uptr, cams, ws, params, out, counter):
    n = len(depths)
    xyz, rgb, view, pixel = out
    dptr, cptr, hw = ptrs
    disp_thresh, num_consistent, depth_min, depth_max = params
    h, w = depths[i].shape
    rc = _launch("fuse_depth_pass", lambda: L.lib().pscv_fuse_depth_pass(
        int(i), dptr, cptr, uptr, hw, n, _p(cams), float(disp_thresh), int(num_consistent), float(depth_min), float(depth_max),
        _p(xyz), _p(rgb), _p(view), _p(pixel), int(xyz.shape[0]), _p(counter), _p(ws), int(ws.numel()), _stream()),
        # per (pixel, other view): one depth gather (4 B) + one colour gather (4 B) at most; ~80 flops
        cost=lambda: (float(h * w * (n - 1) * 8), 80.0 * h * w * (n - 1)))
    L.check(rc, "pscv_fuse_depth_pass")


def _fuse_out(capacity, device, want_view=True):
    xyz = torch.empty((capacity, 3), dtype=torch.float32, device=device)
    rgb = torch.empty((capacity, 3), dtype=torch.uint8, device=device)
    view = torch.empty((capacity,), dtype=torch.int32, device=device) if want_view else None
    pixel = torch.empty((capacity,), dtype=torch.int32, device=device)
    return xyz, rgb, view, pixel


def _fuse_total(counter, capacity, what):
    total = int(counter.item())
    if total > capacity:
        raise L.PscvError(f"{what}: {total} points do not fit the output capacity of {capacity} (nothing past it was written)")
    return total


def fuse_depth_pass(i: int, depths: Sequence[torch.Tensor], colors: Sequence[torch.Tensor], cams: torch.Tensor,
                    used: Sequence[torch.Tensor], *, disp_thresh: float = 0.01, num_consistent: int = 3, depth_min: float = 1e-3,
                    depth_max: float = 1e5, capacity: Optional[int] = None):
    """Pass ``i`` of ``fuse_depth_maps`` alone: depths N x fp32 [h_v,w_v], colors N x uint8 [h_v,w_v,3], cams [N,30]
    (``geo_filter_cams``), used N x uint8 [h_v,w_v] (updated in place), all on the GPU -> the points the pass emits, in row-major
    pixel order: (xyz fp32 [M,3], rgb uint8 [M,3], pixel int32 [M] = y w_i + x).  ``capacity`` (default h_i w_i, the most a pass can
    emit) is the size of the output buffer; a pass that needs more raises ``PscvError``."""
    depths, packed, cams, ptrs, ws = _fuse_inputs(depths, colors, cams)
    _check_used(used, depths)
    if not 0 <= i < len(depths):
        raise ValueError(f"pscv.fuse_depth_pass: pass {i} outside [0,{len(depths)})")
    cap = int(depths[i].numel()) if capacity is None else int(capacity)
    out = _fuse_out(cap, cams.device, want_view=False)
    counter = torch.zeros(1, dtype=torch.int64, device=cams.device)
    _fuse_pass(i, depths, ptrs, _ptrs(used), cams, ws, (disp_thresh, num_consistent, depth_min, depth_max), out, counter)
    m = _fuse_total(counter, cap, "pscv.fuse_depth_pass")
    return out[0][:m], out[1][:m], out[3][:m]


def fuse_depth_maps(depths: Sequence[torch.Tensor], colors: Sequence[torch.Tensor], cams: torch.Tensor, *, disp_thresh: float = 0.01,
                    num_consistent: int = 3, depth_min: float = 1e-3, depth_max: float = 1e5, capacity: Optional[int] = None,
                    want_pixel: bool = False):
    """Consistency fusion of N filtered depth maps into one point cloud (the fusibile step of the
    reference's pipeline): depths N x fp32 [h_v,w_v] (masked pixels 0), colors N x uint8 [h_v,w_v,3], cams [N,30]
    (``geo_filter_cams``; intrinsics at each map's size), all on the GPU, 2 <= N <= 64 -> (xyz fp32 [M,3], rgb uint8 [M,3],
    view int32 [M]) on the GPU, pass-major then row-major pixel order, bit-reproducible.  N passes of pscv_fuse_depth_pass on the
    current stream with the running count on the device; the host reads it once at the end.  ``capacity`` (default: the total
    pixel count, which no run can exceed) sizes the output buffer; a run that needs more raises ``PscvError``.  ``want_pixel``
    appends the pixel index (y w_v + x) each point was emitted from."""
    depths, packed, cams, ptrs, ws = _fuse_inputs(depths, colors, cams)
    dev = cams.device
    used = [torch.zeros(d.shape, dtype=torch.uint8, device=dev) for d in depths]
    uptr = _ptrs(used)
    cap = sum(int(d.numel()) for d in depths) if capacity is None else int(capacity)
    out = _fuse_out(cap, dev)
    counter = torch.zeros(1, dtype=torch.int64, device=dev)
    params = (disp_thresh, num_consistent, depth_min, depth_max)
    for i in range(len(depths)):
        _fuse_pass(i, depths, ptrs, uptr, cams, ws, params, out, counter)
    m = _fuse_total(counter, cap, "pscv.fuse_depth_maps")
    res = (out[0][:m], out[1][:m], out[2][:m])
    return res + (out[3][:m],) if want_pixel else res


# --------------------------------------------------------------------------------------------
# COLMAP-style stereo fusion (the YFCC path: utils/colmap_utils.py:colmap_fusion)
# --------------------------------------------------------------------------------------------
def colmap_overlap_lists(overlap, n: int) -> List[List[int]]:
    """N lists of view indices (or an N x N boolean matrix, row k = the views that follow k, in index order) -> N lists without
    the diagonal or repeats, range-checked."""
    if hasattr(overlap, "shape") and len(overlap.shape) == 2:
        a = np.asarray(overlap.cpu() if torch.is_tensor(overlap) else overlap).astype(bool)
        if a.shape != (n, n):
            raise ValueError(f"pscv.colmap_fuse: overlap matrix must be {n}x{n}, got {a.shape}")
        overlap = [np.nonzero(row)[0].tolist() for row in a]
    if len(overlap) != n:
        raise ValueError(f"pscv.colmap_fuse: {n} overlap lists expected, got {len(overlap)}")
    out = []
    for k, lst in enumerate(overlap):
        seen, row = set(), []
        for m in lst:
            m = int(m)
            if not 0 <= m < n:
                raise ValueError(f"pscv.colmap_fuse: overlap[{k}] names view {m} outside [0,{n})")
            if m != k and m not in seen:
                seen.add(m)
                row.append(m)
        out.append(row)
    return out


def find_next_image_order(overlap: Sequence[Sequence[int]]) -> List[int]:
    """COLMAP's FindNextImage order over all views: after view ``prev`` the first view of ``overlap[prev]`` not yet processed,
    else the lowest-index view not yet processed."""
    n = len(overlap)
    done = [False] * n
    order, prev = [], -1
    for _ in range(n):
        nxt = next((m for m in overlap[prev] if not done[m]), None) if prev >= 0 else None
        if nxt is None:
            nxt = min(v for v in range(n) if not done[v])
        order.append(nxt)
        done[nxt] = True
        prev = nxt
    return order


def _colmap_check(n, max_depth_error, max_reproj_error, min_num_pixels, max_traversal_depth, max_num_pixels):
    if not 2 <= n <= L.FUSE_MAX_VIEWS:
        raise ValueError(f"pscv.colmap_fuse: 2..{L.FUSE_MAX_VIEWS} views expected (PSCV_FUSE_MAX_VIEWS), got {n}")
    if not 0.0 < float(np.float32(max_reproj_error)) <= 2.0:
        raise ValueError(f"pscv.colmap_fuse: max_reproj_error must lie in (0, 2] pixels, got {max_reproj_error}")
    if not 0.0 < float(np.float32(max_depth_error)) < 1.0:
        raise ValueError(f"pscv.colmap_fuse: max_depth_error must lie in (0, 1), got {max_depth_error}")
    if int(min_num_pixels) < 1:
        raise ValueError(f"pscv.colmap_fuse: min_num_pixels must be >= 1, got {min_num_pixels}")
    if int(max_traversal_depth) < 1:
        raise ValueError(f"pscv.colmap_fuse: max_traversal_depth must be >= 1, got {max_traversal_depth}")
    window = (2 * int(math.ceil(float(np.float32(max_reproj_error)))) + 1) ** 2
    if int(max_num_pixels) < 1 + (n - 1) * window:
        raise ValueError(f"pscv.colmap_fuse: max_num_pixels={max_num_pixels} < 1 + (N-1) x window = {1 + (n - 1) * window}: "
                         "COLMAP's cap could cut a cluster, which the parallel rule does not model")


def _colmap_normals(normals, max_normal_error, depths, what):
    """The normal maps of ``colmap_fuse`` checked against the depth maps -> (the list or None, max_normal_error or None)."""
    if (normals is None) != (max_normal_error is None):
        raise ValueError(f"{what}: normals and max_normal_error go together (both, or neither for the constant normals of the "
                         "network path)")
    if normals is None:
        return None, None
    e = float(np.float32(max_normal_error))
    if not 0.0 < e <= 180.0:                         # (false for NaN)
        raise ValueError(f"{what}: max_normal_error must lie in (0, 180] degrees, got {max_normal_error}")
    normals = list(normals)
    if len(normals) != len(depths):
        raise ValueError(f"{what}: one normal map per view expected, got {len(normals)} for {len(depths)} depth maps")
    for v, (nm, d) in enumerate(zip(normals, depths)):
        if not torch.is_tensor(nm) or nm.dtype != torch.float32 or tuple(nm.shape) != tuple(d.shape) + (3,):
            raise ValueError(f"{what}: normal map {v} must be fp32 {tuple(d.shape) + (3,)} (the depth map's size), got "
                             f"{getattr(nm, 'dtype', type(nm))} {tuple(getattr(nm, 'shape', ()))}")
        _dev(nm)
        if nm.device != d.device:
            raise ValueError(f"{what}: normal map {v} is on {nm.device}, its depth map on {d.device}")
    return normals, e


class _ColmapRun:
    """Device state shared by the passes of one fusion: packed inputs, fused masks, claim maps, workspace, output, counter; with
    ``normals`` (N x fp32 [h_v,w_v,3]) and ``max_normal_error`` (degrees) the passes run pscv_colmap_fuse_pass_normals."""

    def __init__(self, depths, colors, cams, overlap, fused, capacity, params, *, normals=None, max_normal_error=None):
        self.depths, self.packed, self.cams, ptrs, _ = _fuse_inputs(depths, colors, cams)
        n = len(self.depths)
        _colmap_check(n, *params)
        self.normals, self.max_normal_error = _colmap_normals(normals, max_normal_error, self.depths, "pscv.colmap_fuse")
        self.nptr = None if self.normals is None else _ptrs(self.normals)
        self.params = params
        self.overlap = colmap_overlap_lists(overlap, n)
        self.bits = (C.c_long * n)(*[C.c_long(sum(1 << m for m in row)).value for row in self.overlap])
        self.dptr, self.cptr, self.hw = ptrs
        dev = self.cams.device
        if fused is None:
            fused = [torch.zeros(d.shape, dtype=torch.uint8, device=dev) for d in self.depths]
        _check_used(fused, self.depths)
        self.fused = fused
        self.fptr = _ptrs(fused)
        self.claim = [torch.full(d.shape, -1, dtype=torch.int64, device=dev) for d in self.depths]
        self.clptr = _ptrs(self.claim)
        ws_bytes = max(int(L.lib().pscv_colmap_fuse_workspace(int(d.shape[0]), int(d.shape[1]))) for d in self.depths)
        self.ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        self.cap = sum(int(d.numel()) for d in self.depths) if capacity is None else int(capacity)
        self.xyz, self.rgb, self.view, self.pixel = _fuse_out(self.cap, dev)
        self.normal = torch.empty((self.cap, 3), dtype=torch.float32, device=dev)
        self.counter = torch.zeros(1, dtype=torch.int64, device=dev)

    def run_pass(self, view: int, tag: int, processed: int):
        n = len(self.depths)
        e, r, mnp, mtd, _ = self.params
        h, w = self.depths[view].shape
        if self.normals is not None:
            rc = _launch("colmap_fuse_pass_normals", lambda: L.lib().pscv_colmap_fuse_pass_normals(
                int(view), int(tag), self.dptr, self.cptr, self.fptr, self.clptr, self.hw, n, _p(self.cams), self.bits,
                C.c_long(int(processed)).value, float(e), float(r), int(mnp), int(mtd), self.nptr, float(self.max_normal_error),
                _p(self.xyz), _p(self.normal), _p(self.rgb), _p(self.view), _p(self.pixel), self.cap, _p(self.counter), _p(self.ws),
                int(self.ws.numel()), _stream()),
                # as below, plus 12 B of normal per window pixel that passed depth and reprojection (phase A, at most all) and per
                # cluster node (phase B)
                cost=lambda: (float(h * w * (n - 1) * (2 * 25 * 5 + 2 * 25 * 12)), 0.0))
            L.check(rc, "pscv_colmap_fuse_pass_normals")
            return
        rc = _launch("colmap_fuse_pass", lambda: L.lib().pscv_colmap_fuse_pass(
            int(view), int(tag), self.dptr, self.cptr, self.fptr, self.clptr, self.hw, n, _p(self.cams), self.bits, C.c_long(int(processed)).value,
            float(e), float(r), int(mnp), int(mtd), _p(self.xyz), _p(self.normal), _p(self.rgb), _p(self.view), _p(self.pixel),
            self.cap, _p(self.counter), _p(self.ws), int(self.ws.numel()), _stream()),
            # per (seed, other view): one window of depth + mask reads, twice (phases A and B)
            cost=lambda: (float(h * w * (n - 1) * 2 * 25 * 5), 0.0))
        L.check(rc, "pscv_colmap_fuse_pass")

    def result(self, what):
        m = _fuse_total(self.counter, self.cap, what)
        return self.xyz[:m], self.normal[:m], self.rgb[:m], self.view[:m], self.pixel[:m]


def colmap_fuse_pass(view: int, depths: Sequence[torch.Tensor], colors: Sequence[torch.Tensor], cams: torch.Tensor, overlap,
                     fused: Sequence[torch.Tensor], *, processed: Sequence[int] = (), max_depth_error: float = 0.01,
                     max_reproj_error: float = 1.0, min_num_pixels: int = 3, max_traversal_depth: int = 100,
                     max_num_pixels: int = 10000, capacity: Optional[int] = None,
                     normals: Optional[Sequence[torch.Tensor]] = None, max_normal_error: Optional[float] = None):
    """The pass of view ``view`` of ``colmap_fuse`` alone, with explicit state: ``fused`` N x uint8 [h_v,w_v] masks (updated in
    place) and ``processed`` the views whose passes are done -> (xyz fp32 [M,3], normal fp32 [M,3], rgb uint8 [M,3], pixel int32
    [M] = y w + x of each seed), row-major seed order.  ``capacity`` (default h w of the view) sizes the output buffer; a pass that
    needs more raises ``PscvError``.  ``normals`` / ``max_normal_error`` as in ``colmap_fuse``."""
    n = len(depths)
    if not 0 <= int(view) < n:
        raise ValueError(f"pscv.colmap_fuse_pass: view {view} outside [0,{n})")
    proc = 0
    for v in processed:
        if not 0 <= int(v) < n or int(v) == int(view):
            raise ValueError(f"pscv.colmap_fuse_pass: processed view {v} invalid for the pass of view {view}")
        proc |= 1 << int(v)
    cap = int(depths[view].numel()) if capacity is None else int(capacity)
    run = _ColmapRun(depths, colors, cams, overlap, list(fused), cap,
                     (max_depth_error, max_reproj_error, min_num_pixels, max_traversal_depth, max_num_pixels),
                     normals=normals, max_normal_error=max_normal_error)
    run.run_pass(int(view), 0, proc)
    xyz, normal, rgb, _, pixel = run.result("pscv.colmap_fuse_pass")
    return xyz, normal, rgb, pixel


def colmap_fuse(depths: Sequence[torch.Tensor], colors: Sequence[torch.Tensor], cams: torch.Tensor, overlap, *, max_depth_error: float,
                max_reproj_error: float, min_num_pixels: int, max_traversal_depth: int = 100, max_num_pixels: int = 10000,
                capacity: Optional[int] = None, want_pixel: bool = False,
                normals: Optional[Sequence[torch.Tensor]] = None, max_normal_error: Optional[float] = None):
    """COLMAP-style stereo fusion of N depth maps into one point cloud (the YFCC fusion of the
    reference's pipeline): depths N x fp32 [h_v,w_v] (masked pixels 0), colors N x uint8 [h_v,w_v,3], cams [N,30]
    (``geo_filter_cams``; intrinsics at each map's size), all on the GPU, 2 <= N <= 64; overlap N lists of view indices (COLMAP's
    overlapping images, best first) or an N x N boolean matrix -> (xyz fp32 [M,3], normal fp32 [M,3], rgb uint8 [M,3], view int32
    [M]) on the GPU, pass-major (FindNextImage order, computed on the host) then row-major seed order, bit-reproducible.  One
    pscv_colmap_fuse_pass per view on the current stream; the host reads the point count once at the end.  ``capacity`` (default:
    the total pixel count, which no run can exceed) sizes the output; a run that needs more raises ``PscvError``.  ``want_pixel``
    appends the seed pixel index (y w_v + x) of each point.

    Without ``normals`` every view has the constant normal of the reference's network path and the normal test is off.  With
    ``normals`` (N x fp32 [h_v,w_v,3] on the GPU, contiguous: unit normals in the camera frame of their view, 0 where the depth is
    filtered, what ``patch_match_filter`` returns) and ``max_normal_error`` (degrees, in (0, 180]) a pixel joins a seed only when
    their world normals are within that angle, and the fused normal is the normalised per-component median over the cluster
    (section 2g, "with normal maps"; pscv_colmap_fuse_pass_normals).  One without the other is a ``ValueError``."""
    run = _ColmapRun(depths, colors, cams, overlap, None, capacity,
                     (max_depth_error, max_reproj_error, min_num_pixels, max_traversal_depth, max_num_pixels),
                     normals=normals, max_normal_error=max_normal_error)
    processed = 0
    for tag, v in enumerate(find_next_image_order(run.overlap)):
        run.run_pass(v, tag, processed)
        processed |= 1 << v
    xyz, normal, rgb, view, pixel = run.result("pscv.colmap_fuse")
    res = (xyz, normal, rgb, view)
    return res + (pixel,) if want_pixel else res


def view_covisibility(depths: Sequence[torch.Tensor], cams: torch.Tensor, *, stride: int = 4, max_depth_error: float) -> torch.Tensor:
    """Which views see the same surface, from the depth maps alone ("Overlap without a sparse model"):
    depths V x fp32 [h_v,w_v] (0 = invalid), cams [V,30] (``geo_filter_cams``; intrinsics at each map's size), on the GPU, V >= 2
    with no upper bound -> int32 [V,V,2] on the GPU.  ``[v,u,0]`` counts the samples of v (every ``stride``-th row and column with a
    valid depth) that project inside u's map at a positive depth, ``[v,u,1]`` those whose depth there agrees with u's map within
    ``max_depth_error`` (relative); pixel, rounding and depth test are those of phase A of ``colmap_fuse``.  The diagonal is 0.  One
    pscv_view_covisibility call on the current stream, no host synchronisation; ``utils.colmap_model.overlap_from_covisibility``
    turns the counts into the overlap lists of ``colmap_fuse``."""
    what = "pscv.view_covisibility"
    depths, cams = _view_maps(what, depths, cams, lo=0, cast=True)         # (the C entry point refuses V < 2)
    dev = _one_device(what, "depth maps and cams", cams, *depths)
    n, dptr, hw = len(depths), _ptrs(depths), _hw(depths)
    counts = torch.empty((n, n, 2), dtype=torch.int32, device=dev)
    ws = torch.empty(max(int(L.lib().pscv_view_covisibility_workspace(n)), 1), dtype=torch.uint8, device=dev)
    samples = sum(-(-d.shape[0] // max(int(stride), 1)) * -(-d.shape[1] // max(int(stride), 1)) for d in depths)
    rc = _launch("view_covisibility", lambda: L.lib().pscv_view_covisibility(
        dptr, hw, n, _p(cams), int(stride), float(max_depth_error), _p(counts), _p(ws), int(ws.numel()), _stream()),
        # per (sample, target): one depth gather at most; ~45 fp64 operations (projection, two divisions, the depth test)
        cost=lambda: (float(samples * (n - 1) * 4), 45.0 * samples * (n - 1)))
    L.check(rc, "pscv_view_covisibility")
    return counts


# --------------------------------------------------------------------------------------------
# normal maps from depth maps (the normals of a network reconstruction)
# --------------------------------------------------------------------------------------------
DEPTH_NORMALS_MAX_RADIUS = 4


def depth_normals(depths: Sequence[torch.Tensor], cams: torch.Tensor, *, radius: int = 2, rel_gate: float = 0.05,
                  min_support: int = 6, want_support: bool = False):
    """Normal maps from depth maps: depths V x fp32 [h_v,w_v] (0 = invalid), cams [V,30]
    (``geo_filter_cams``; intrinsics at each map's size), on the GPU, any V -> V x fp32 [h_v,w_v,3] on the GPU: unit normals in
    the camera frame of their view facing the camera (n^T K^-1 p < 0), 0 at invalid pixels -- what ``colmap_fuse(normals=...)``
    takes.  Per valid pixel a least-squares fit of the inverse depth over the (2 ``radius`` + 1)^2 window (``radius`` 1..4), over
    the taps within ``rel_gate`` (relative) of the centre's depth; with fewer than ``min_support`` taps (3..window), collinear
    taps or a fit that faces away, the pixel gets the ray towards the camera.  ``want_support`` appends V x int32 [h_v,w_v]: the
    tap count, negated where the pixel fell back, 0 where invalid.  One pscv_depth_normals launch per 64 views on the current
    stream, no host synchronisation, bit-reproducible."""
    what = "pscv.depth_normals"
    r = int(radius)
    if not 1 <= r <= DEPTH_NORMALS_MAX_RADIUS:
        raise ValueError(f"{what}: radius must lie in [1, {DEPTH_NORMALS_MAX_RADIUS}], got {radius}")
    tau = float(rel_gate)
    if not (tau > 0.0 and math.isfinite(tau)):                    # (false for NaN)
        raise ValueError(f"{what}: rel_gate must be positive and finite, got {rel_gate}")
    window = (2 * r + 1) ** 2
    if not 3 <= int(min_support) <= window:
        raise ValueError(f"{what}: min_support must lie in [3, {window}] (the window of radius {r}), got {min_support}")
    depths, cams = _view_maps(what, depths, cams, lo=0, cast=True)
    dev = _one_device(what, "depth maps and cams", cams, *depths)
    normals = [torch.empty(tuple(d.shape) + (3,), dtype=torch.float32, device=dev) for d in depths]
    supports = [torch.empty(d.shape, dtype=torch.int32, device=dev) for d in depths] if want_support else None
    for part, k, dptr, hw, cam_part in _view_chunks(depths, cams):
        pixels = sum(int(d.numel()) for d in depths[part])
        rc = _launch("depth_normals", lambda: L.lib().pscv_depth_normals(
            dptr, hw, k, _p(cam_part), r, tau, int(min_support), _ptrs(normals[part]),
            None if supports is None else _ptrs(supports[part]), _stream()),
            # per pixel: 4 B read, 12 (+ 4) B written; per tap ~12 fp64 operations
            cost=lambda: (float(pixels * (20 if want_support else 16)), 12.0 * window * pixels))
        L.check(rc, "pscv_depth_normals")
    return (normals, supports) if want_support else normals


def point_world_normals(view: torch.Tensor, pixel: torch.Tensor, normals: Sequence[torch.Tensor], cams: torch.Tensor) -> torch.Tensor:
    """World normals of fused points: view, pixel int32 [M] (the emitting view and pixel y w_v + x of each point, what
    ``fuse_depth_maps(want_pixel=True)`` and ``colmap_fuse(want_pixel=True)`` return), normals V x fp32 [h_v,w_v,3] (camera
    frame, ``depth_normals``), cams [V,30], on the GPU, 1 <= V <= 64 -> fp32 [M,3] on the GPU, ``R_v^T n`` by the rule of the
    fusion's normal test (fp64 sums rounded to fp32).  An index outside its range gives (0,0,0).  One launch, no host
    synchronisation."""
    what = "pscv.point_world_normals"
    normals = list(normals)
    n = len(normals)
    if not 1 <= n <= L.FUSE_MAX_VIEWS:
        raise ValueError(f"{what}: 1..{L.FUSE_MAX_VIEWS} normal maps expected (PSCV_FUSE_MAX_VIEWS), got {n}")
    for v, nm in enumerate(normals):
        if not torch.is_tensor(nm) or nm.dtype != torch.float32 or nm.dim() != 3 or nm.shape[2] != 3:
            raise ValueError(f"{what}: normal map {v} must be fp32 [h,w,3], got {getattr(nm, 'dtype', type(nm))} "
                             f"{tuple(getattr(nm, 'shape', ()))}")
    for name, idx in (("view", view), ("pixel", pixel)):
        if not torch.is_tensor(idx) or idx.dtype != torch.int32 or idx.dim() != 1:
            raise ValueError(f"{what}: {name} must be int32 [M], got {getattr(idx, 'dtype', type(idx))} {tuple(getattr(idx, 'shape', ()))}")
    if view.shape != pixel.shape:
        raise ValueError(f"{what}: view and pixel must have one entry per point, got {tuple(view.shape)} and {tuple(pixel.shape)}")
    cams = cams.to(torch.float32).contiguous()
    view, pixel = view.contiguous(), pixel.contiguous()
    _check_cams(cams, n, what)
    dev = _one_device(what, "indices, normal maps and cams", cams, view, pixel, *normals)
    m = int(view.shape[0])
    out = torch.empty((m, 3), dtype=torch.float32, device=dev)
    hw = (C.c_int * (2 * n))(*[s for nm in normals for s in nm.shape[:2]])
    rc = _launch("point_world_normals", lambda: L.lib().pscv_point_world_normals(
        _p(view), _p(pixel), m, _ptrs(normals), hw, n, _p(cams), _p(out), _stream()),
        cost=lambda: (float(m * (8 + 12 + 12)), 15.0 * m))
    L.check(rc, "pscv_point_world_normals")
    return out


# --------------------------------------------------------------------------------------------
# TSDF fusion of depth maps and marching-tetrahedra meshing
# --------------------------------------------------------------------------------------------
TSDF_MAX_VOXELS = 2 ** 31 - 1
TSDF_MAX_VIEWS = (2 ** 24 - 1) // 255          # 65793: rgb_sum holds integers in fp32, exact while 255 cweight < 2^24


@dataclass
class TsdfVolume:
    """The state of a TSDF grid of ``dims`` = (nx, ny, nz) on one GPU: tsdf_sum fp32, weight int32, cweight int32 [nz,ny,nx] and
    rgb_sum fp32 [nz,ny,nx,3]; ``views`` counts the views integrated so far (host side)."""
    dims: tuple
    tsdf_sum: torch.Tensor
    weight: torch.Tensor
    rgb_sum: torch.Tensor
    cweight: torch.Tensor
    views: int = 0

    def arrays(self):
        return self.tsdf_sum, self.weight, self.rgb_sum, self.cweight


def _tsdf_dims(dims, what):
    try:
        nx, ny, nz = (int(v) for v in dims)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: dims must be three integers (nx, ny, nz), got {dims!r}")
    if min(nx, ny, nz) < 1 or nx * ny * nz > TSDF_MAX_VOXELS:
        raise ValueError(f"{what}: dims {nx} x {ny} x {nz} must be positive with nx ny nz < 2^31")
    return nx, ny, nz


def _tsdf_grid(origin, voxel, what):
    try:
        o = tuple(float(v) for v in origin)
    except (TypeError, ValueError):
        o = ()
    if len(o) != 3 or not all(math.isfinite(v) for v in o):
        raise ValueError(f"{what}: origin must be three finite numbers, got {origin!r}")
    s = float(voxel)
    if not (s > 0.0 and math.isfinite(s)):
        raise ValueError(f"{what}: voxel must be positive and finite, got {voxel}")
    return o, s


def _trunc(trunc, what):
    tr = float(trunc)
    if not (tr > 0.0 and math.isfinite(tr)):
        raise ValueError(f"{what}: trunc must be positive and finite, got {trunc}")
    return tr


def _tsdf_room(volume, n, what):
    if volume.views + n > TSDF_MAX_VIEWS:
        raise ValueError(f"{what}: {volume.views} + {n} views exceed the {TSDF_MAX_VIEWS} a volume can hold (its fp32 colour sums stay "
                         f"exact only while 255 cweight < 2^24)")


def _tsdf_state(state, what):
    if not isinstance(state, TsdfVolume):
        raise ValueError(f"{what}: state must be the TsdfVolume of ops.tsdf_volume, got {type(state).__name__}")
    nx, ny, nz = _tsdf_dims(state.dims, what)
    want = ((torch.float32, (nz, ny, nx)), (torch.int32, (nz, ny, nx)), (torch.float32, (nz, ny, nx, 3)), (torch.int32, (nz, ny, nx)))
    for name, t, (dt, shape) in zip(("tsdf_sum", "weight", "rgb_sum", "cweight"), state.arrays(), want):
        if not torch.is_tensor(t) or t.dtype != dt or tuple(t.shape) != shape:
            raise ValueError(f"{what}: state.{name} must be {dt} {shape}, got {getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))}")
    return nx, ny, nz


def tsdf_volume(dims, device="cuda") -> TsdfVolume:
    """The zeroed state of a TSDF grid of ``dims`` = (nx, ny, nz), nx ny nz < 2^31, on ``device`` (24 bytes per voxel)."""
    nx, ny, nz = _tsdf_dims(dims, "pscv.tsdf_volume")
    z = lambda dt, *more: torch.zeros((nz, ny, nx) + more, dtype=dt, device=device)
    return TsdfVolume((nx, ny, nz), z(torch.float32), z(torch.int32), z(torch.float32, 3), z(torch.int32))


def _max_valid_depth(depths):
    """fp32 [V] on the device: the largest valid (0 < d finite) depth of each map, 0 for a map without one (plumbing: no host read)."""
    def amax(d):
        ok = (d > 0) & (d <= torch.finfo(torch.float32).max)
        return torch.where(ok, d, torch.zeros_like(d)).flatten(-2).amax(dim=-1)
    if all(d.shape == depths[0].shape for d in depths):
        return amax(torch.stack(depths)).contiguous()
    return torch.stack([amax(d) for d in depths]).contiguous()


def tsdf_integrate(state: TsdfVolume, depths: Sequence[torch.Tensor], colors: Sequence[torch.Tensor], cams: torch.Tensor, *,
                   origin, voxel: float, trunc: float) -> TsdfVolume:
    """Integrates depth maps into the TSDF ``state`` in place: depths V x fp32 [h_v,w_v] (0 = invalid),
    colors V x uint8 [h_v,w_v,3] (or packed int32 [h_v,w_v], ``pack_rgba8``), cams [V,30] (``geo_filter_cams``), on the GPU of the
    state, any V >= 1.  Lattice point (i,j,k) sits at ``origin`` + (i,j,k) ``voxel``; per voxel and view the signed distance along
    the view's z axis, sd = d - z at the pixel the voxel's centre rounds to, is kept when sd >= -``trunc`` and adds min(1, sd /
    trunc) to tsdf_sum and 1 to weight; where also sd <= trunc the pixel's colour joins rgb_sum / cweight.  One
    pscv_tsdf_integrate launch per 64 views in view order on the current stream, no host synchronisation, bit-reproducible."""
    what = "pscv.tsdf_integrate"
    nx, ny, nz = _tsdf_state(state, what)
    o, s = _tsdf_grid(origin, voxel, what)
    tr = _trunc(trunc, what)
    depths, cams = _view_maps(what, depths, cams, lo=1, cast=False)
    packed = _view_colors(what, depths, colors)
    _tsdf_room(state, len(depths), what)
    _one_device(what, "state, depth maps, colours and cams", *state.arrays(), cams, *depths, *packed)
    for part, k, dptr, hw, cam_part in _view_chunks(depths, cams):
        dmax = _max_valid_depth(depths[part])
        rc = _launch("tsdf_integrate", lambda: L.lib().pscv_tsdf_integrate(
            dptr, _ptrs(packed[part]), hw, k, _p(cam_part), _p(dmax), o[0], o[1], o[2], s, tr, nx, ny, nz,
            _p(state.tsdf_sum), _p(state.weight), _p(state.rgb_sum), _p(state.cweight), _stream()),
            # the state read and written once (2 x 24 B per voxel); per voxel and view ~60 fp64 operations and three divisions
            cost=lambda: (48.0 * nx * ny * nz, 100.0 * nx * ny * nz * k))
        L.check(rc, "pscv_tsdf_integrate")
        state.views += k
    return state


def tsdf_extract(state: TsdfVolume, *, origin, voxel: float, min_weight: int = 1):
    """Marching tetrahedra over the TSDF ``state`` -> (xyz fp32 [V,3], rgb uint8 [V,3], faces int32
    [F,3]) on the GPU: the zero crossing of f = tsdf_sum / weight over the voxels with weight >= ``min_weight`` (>= 1), one vertex
    per sign-changing lattice edge (ordered by voxel, then edge type), faces oriented towards the positive (free-space) side,
    ordered by cell and tetrahedron.  Mark, two prefix sums (torch), one host read of their last entries (the totals), two emits; bit-reproducible."""
    what = "pscv.tsdf_extract"
    nx, ny, nz = _tsdf_state(state, what)
    o, s = _tsdf_grid(origin, voxel, what)
    if isinstance(min_weight, bool) or int(min_weight) != min_weight or int(min_weight) < 1:
        raise ValueError(f"{what}: min_weight must be an integer >= 1, got {min_weight!r}")
    _dev(*state.arrays())
    dev = state.tsdf_sum.device
    nvox = nx * ny * nz
    info = torch.empty(nvox, dtype=torch.int32, device=dev)
    st = _stream()
    rc = _launch("tsdf_mark", lambda: L.lib().pscv_tsdf_mark(_p(state.tsdf_sum), _p(state.weight), nx, ny, nz, int(min_weight),
                                                             _p(info), st), cost=lambda: (12.0 * nvox, 2.0 * nvox))
    L.check(rc, "pscv_tsdf_mark")
    counts = info.view(torch.uint8).view(nvox, 4)[:, 2:]              # (little-endian: byte 2 = vertices, byte 3 = faces)
    if 12 * nvox >= 2 ** 31:       # a voxel has at most 7 vertices and 12 faces: only a grid this large can overflow the int32 sums
        totals = counts.sum(dim=0, dtype=torch.int64).tolist()
        if max(totals) >= 2 ** 31:
            raise L.PscvError(f"{what}: {totals[0]} vertices and {totals[1]} faces do not fit int32 indices")
    vincl = torch.cumsum(counts[:, 0], dim=0, dtype=torch.int32)
    fincl = torch.cumsum(counts[:, 1], dim=0, dtype=torch.int32)
    n_vert, n_face = (int(v) for v in torch.stack((vincl[-1], fincl[-1])).tolist())   # the totals: the one host read
    xyz = torch.empty((n_vert, 3), dtype=torch.float32, device=dev)
    rgb = torch.empty((n_vert, 3), dtype=torch.uint8, device=dev)
    faces = torch.empty((n_face, 3), dtype=torch.int32, device=dev)
    if n_vert == 0:
        return xyz, rgb, faces
    rc = _launch("tsdf_emit_vertices", lambda: L.lib().pscv_tsdf_emit_vertices(
        _p(state.tsdf_sum), _p(state.weight), _p(state.rgb_sum), _p(state.cweight), _p(info), _p(vincl), nx, ny, nz, o[0], o[1], o[2],
        s, _p(xyz), _p(rgb), n_vert, st), cost=lambda: (8.0 * nvox + 60.0 * n_vert, 40.0 * n_vert))
    L.check(rc, "pscv_tsdf_emit_vertices")
    if n_face:
        rc = _launch("tsdf_emit_faces", lambda: L.lib().pscv_tsdf_emit_faces(_p(info), _p(vincl), _p(fincl), nx, ny, nz, _p(faces),
                                                                             n_face, st), cost=lambda: (8.0 * nvox + 12.0 * n_face, 0.0))
        L.check(rc, "pscv_tsdf_emit_faces")
    return xyz, rgb, faces


# --------------------------------------------------------------------------------------------
# the same volume as a pool of 8 x 8 x 8 bricks behind a dense directory
# --------------------------------------------------------------------------------------------
TSDF_BRICK = 8
TSDF_MAX_BRICKS = 2 ** 22 - 1                  # a pool voxel index (slot 512 + local) fits int32
TSDF_BRICK_BYTES = 24 * TSDF_BRICK ** 3        # the state of one brick


@dataclass
class TsdfBricks:
    """A TSDF lattice of ``dims`` = (nx, ny, nz) stored as n bricks of 8 x 8 x 8: ``directory`` int32 [nbz,nby,nbx] (the brick's pool
    slot, -1 = not allocated), ``brick_ids`` int32 [n] (the brick of every slot, ascending), the pool arrays tsdf_sum fp32, weight
    int32, cweight int32 [n,8,8,8] and rgb_sum fp32 [n,8,8,8,3]; ``views`` counts the views integrated so far (host side)."""
    dims: tuple
    directory: torch.Tensor
    brick_ids: torch.Tensor
    tsdf_sum: torch.Tensor
    weight: torch.Tensor
    rgb_sum: torch.Tensor
    cweight: torch.Tensor
    views: int = 0

    def arrays(self):
        return self.tsdf_sum, self.weight, self.rgb_sum, self.cweight


def _brick_dims(dims, what):
    """(nx, ny, nz), (nbx, nby, nbz): the lattice may exceed 2^31 points, the directory may not."""
    try:
        nx, ny, nz = (int(v) for v in dims)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: dims must be three integers (nx, ny, nz), got {dims!r}")
    if min(nx, ny, nz) < 1 or max(nx, ny, nz) > 2 ** 31 - 1 - TSDF_BRICK:
        raise ValueError(f"{what}: dims {nx} x {ny} x {nz} must be positive int32")
    nb = tuple(-(-n // TSDF_BRICK) for n in (nx, ny, nz))
    if nb[0] * nb[1] * nb[2] >= 2 ** 31:
        raise ValueError(f"{what}: dims {nx} x {ny} x {nz} need {nb[0]} x {nb[1]} x {nb[2]} bricks: nbx nby nbz must stay below 2^31")
    return (nx, ny, nz), nb


def _min_valid_depth(depths):
    """fp32 [V] on the device: the smallest valid (0 < d finite) depth of each map, +inf for a map without one (plumbing)."""
    def amin(d):
        ok = (d > 0) & (d <= torch.finfo(torch.float32).max)
        return torch.where(ok, d, torch.full_like(d, float("inf"))).flatten(-2).amin(dim=-1)
    if all(d.shape == depths[0].shape for d in depths):
        return amin(torch.stack(depths)).contiguous()
    return torch.stack([amin(d) for d in depths]).contiguous()


def tsdf_brick_probe(depths: Sequence[torch.Tensor], cams: torch.Tensor, dims, *, origin, voxel: float, trunc: float) -> torch.Tensor:
    """Where the surface can be -> masks int32 [nbz,nby,nbx] on the GPU of the depth maps.  A lattice
    point is touched when some view updates it with -trunc <= sd <= trunc; a touched point at local (x, y, z) of its brick sets bit
    (dz+1) 9 + (dy+1) 3 + (dx+1) of the brick's mask for every neighbour brick (itself included) that holds one of its 26
    neighbours.  No state is read; one pscv_tsdf_brick_probe launch per 64 views, no host synchronisation."""
    what = "pscv.tsdf_brick_probe"
    (nx, ny, nz), nb = _brick_dims(dims, what)
    o, s = _tsdf_grid(origin, voxel, what)
    tr = _trunc(trunc, what)
    depths, cams = _view_maps(what, depths, cams, lo=1, cast=False)
    dev = _one_device(what, "depth maps and cams", cams, *depths)
    masks = torch.zeros(nb[::-1], dtype=torch.int32, device=dev)
    nbricks = nb[0] * nb[1] * nb[2]
    for part, k, dptr, hw, cam_part in _view_chunks(depths, cams):
        dmax, dmin = _max_valid_depth(depths[part]), _min_valid_depth(depths[part])
        rc = _launch("tsdf_brick_probe", lambda: L.lib().pscv_tsdf_brick_probe(
            dptr, hw, k, _p(cam_part), _p(dmax), _p(dmin), o[0], o[1], o[2], s, tr, nx, ny, nz, _p(masks), _stream()),
            cost=lambda: (8.0 * nbricks, 100.0 * nbricks * k))
        L.check(rc, "pscv_tsdf_brick_probe")
    return masks


def tsdf_bricks(masks: torch.Tensor, dims, max_bricks=None) -> TsdfBricks:
    """The zeroed brick volume for the masks of ``tsdf_brick_probe``: brick b is allocated iff some brick b - (dx,dy,dz) has the bit
    of (dx,dy,dz) set (requests that leave the directory are dropped), slots are numbered by ascending brick index.  The shifts,
    the nonzero and the directory are torch plumbing; one host read (the number of bricks) sizes the pool.  More than ``max_bricks``
    (None: no limit of the caller's) or 2^22 - 1 bricks is a ValueError that names the count and the bytes."""
    what = "pscv.tsdf_bricks"
    dims, nb = _brick_dims(dims, what)
    if not torch.is_tensor(masks) or masks.dtype != torch.int32 or tuple(masks.shape) != nb[::-1]:
        raise ValueError(f"{what}: masks must be int32 {nb[::-1]} (tsdf_brick_probe), got {getattr(masks, 'dtype', type(masks))} "
                         f"{tuple(getattr(masks, 'shape', ()))}")
    if max_bricks is not None and (isinstance(max_bricks, bool) or int(max_bricks) != max_bricks or int(max_bricks) < 0):
        raise ValueError(f"{what}: max_bricks must be None or an integer >= 0, got {max_bricks!r}")
    alloc = torch.zeros(masks.shape, dtype=torch.bool, device=masks.device)
    for bit in range(27):
        d = (bit % 3 - 1, bit // 3 % 3 - 1, bit // 9 - 1)                     # (dx, dy, dz)
        src = tuple(slice(max(0, -v), n - max(0, v)) for v, n in zip(d[::-1], masks.shape))
        dst = tuple(slice(max(0, v), n - max(0, -v)) for v, n in zip(d[::-1], masks.shape))
        alloc[dst] |= (masks[src] >> bit & 1).bool()
    brick_ids = torch.nonzero(alloc.reshape(-1)).reshape(-1)                  # (ascending; its size is the one host read)
    n = int(brick_ids.shape[0])
    limit = TSDF_MAX_BRICKS if max_bricks is None else min(int(max_bricks), TSDF_MAX_BRICKS)
    if n > limit:
        raise ValueError(f"{what}: the views ask for {n} bricks ({n * TSDF_BRICK_BYTES} bytes of state), more than "
                         f"{'max_bricks = ' + str(max_bricks) if limit < TSDF_MAX_BRICKS else 'the 2^22 - 1 a pool can hold'}: "
                         f"pass `bounds` or a larger `voxel`")
    brick_ids = brick_ids.to(torch.int32)
    directory = torch.full((alloc.numel(),), -1, dtype=torch.int32, device=masks.device)
    directory[brick_ids.long()] = torch.arange(n, dtype=torch.int32, device=masks.device)
    B = TSDF_BRICK
    z = lambda dt, *more: torch.zeros((n, B, B, B) + more, dtype=dt, device=masks.device)
    return TsdfBricks(dims, directory.reshape(alloc.shape), brick_ids, z(torch.float32), z(torch.int32), z(torch.float32, 3), z(torch.int32))


def _tsdf_brick_state(bricks, what):
    if not isinstance(bricks, TsdfBricks):
        raise ValueError(f"{what}: bricks must be the TsdfBricks of ops.tsdf_bricks, got {type(bricks).__name__}")
    (nx, ny, nz), nb = _brick_dims(bricks.dims, what)
    ids, direc = bricks.brick_ids, bricks.directory
    if not torch.is_tensor(ids) or ids.dtype != torch.int32 or ids.dim() != 1 or ids.shape[0] > TSDF_MAX_BRICKS:
        raise ValueError(f"{what}: bricks.brick_ids must be int32 [n], n < 2^22")
    if not torch.is_tensor(direc) or direc.dtype != torch.int32 or tuple(direc.shape) != nb[::-1]:
        raise ValueError(f"{what}: bricks.directory must be int32 {nb[::-1]}")
    n, B = int(ids.shape[0]), TSDF_BRICK
    want = ((torch.float32, (n, B, B, B)), (torch.int32, (n, B, B, B)), (torch.float32, (n, B, B, B, 3)), (torch.int32, (n, B, B, B)))
    for name, t, (dt, shape) in zip(("tsdf_sum", "weight", "rgb_sum", "cweight"), bricks.arrays(), want):
        if not torch.is_tensor(t) or t.dtype != dt or tuple(t.shape) != shape:
            raise ValueError(f"{what}: bricks.{name} must be {dt} {shape}, got {getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))}")
    return (nx, ny, nz), n


def tsdf_brick_integrate(bricks: TsdfBricks, depths: Sequence[torch.Tensor], colors: Sequence[torch.Tensor], cams: torch.Tensor, *,
                         origin, voxel: float, trunc: float) -> TsdfBricks:
    """``tsdf_integrate`` on every lattice point of every allocated brick, in place: the views in ascending order, one
    pscv_tsdf_brick_integrate launch per 64, tsdf_sum rounded to fp32 once per launch.  The views, origin, voxel and trunc must be
    those the bricks were probed with: a brick allocated for other views would miss free-space updates."""
    what = "pscv.tsdf_brick_integrate"
    (nx, ny, nz), nbr = _tsdf_brick_state(bricks, what)
    o, s = _tsdf_grid(origin, voxel, what)
    tr = _trunc(trunc, what)
    depths, cams = _view_maps(what, depths, cams, lo=1, cast=False)
    packed = _view_colors(what, depths, colors)
    _tsdf_room(bricks, len(depths), what)
    _one_device(what, "bricks, depth maps, colours and cams", *bricks.arrays(), bricks.brick_ids, bricks.directory, cams, *depths, *packed)
    for part, k, dptr, hw, cam_part in _view_chunks(depths, cams):
        dmax = _max_valid_depth(depths[part])
        rc = _launch("tsdf_brick_integrate", lambda: L.lib().pscv_tsdf_brick_integrate(
            dptr, _ptrs(packed[part]), hw, k, _p(cam_part), _p(dmax), o[0], o[1], o[2], s, tr, nx, ny, nz, _p(bricks.brick_ids), nbr,
            _p(bricks.tsdf_sum), _p(bricks.weight), _p(bricks.rgb_sum), _p(bricks.cweight), _stream()),
            cost=lambda: (48.0 * 512 * nbr, 100.0 * 512 * nbr * k))
        L.check(rc, "pscv_tsdf_brick_integrate")
        bricks.views += k
    return bricks


def tsdf_brick_extract(bricks: TsdfBricks, *, origin, voxel: float, min_weight: int = 1, return_keys: bool = False):
    """``tsdf_extract`` over a brick volume -> (xyz fp32 [V,3], rgb uint8 [V,3], faces int32 [F,3]) and, with ``return_keys``, the
    vertices' int64 keys lin(p) 7 + (d - 1) [V].  A voxel outside the lattice or in a brick that is not allocated counts as
    unobserved.  The mesh holds the vertices and triangles of the dense extraction, ordered by (slot, local voxel, edge type) and
    (slot, local cell, tetrahedron); every face starts at its vertex of the smallest key, as the dense faces do."""
    what = "pscv.tsdf_brick_extract"
    (nx, ny, nz), nbr = _tsdf_brick_state(bricks, what)
    o, s = _tsdf_grid(origin, voxel, what)
    if isinstance(min_weight, bool) or int(min_weight) != min_weight or int(min_weight) < 1:
        raise ValueError(f"{what}: min_weight must be an integer >= 1, got {min_weight!r}")
    _dev(*bricks.arrays(), bricks.brick_ids, bricks.directory)
    dev = bricks.tsdf_sum.device
    nvox = nbr * TSDF_BRICK ** 3
    empty = lambda n: (torch.empty((n, 3), dtype=torch.float32, device=dev), torch.empty((n, 3), dtype=torch.uint8, device=dev))
    keys = lambda n: (torch.empty((n,), dtype=torch.int64, device=dev),) if return_keys else ()
    if nbr == 0:
        return empty(0) + (torch.empty((0, 3), dtype=torch.int32, device=dev),) + keys(0)
    info = torch.empty(nvox, dtype=torch.int32, device=dev)
    st = _stream()
    grid = (_p(bricks.directory), _p(bricks.brick_ids), nbr, nx, ny, nz)
    rc = _launch("tsdf_brick_mark", lambda: L.lib().pscv_tsdf_brick_mark(_p(bricks.tsdf_sum), _p(bricks.weight), *grid, int(min_weight),
                                                                         _p(info), st), cost=lambda: (12.0 * nvox, 2.0 * nvox))
    L.check(rc, "pscv_tsdf_brick_mark")
    counts = info.view(torch.uint8).view(nvox, 4)[:, 2:]              # (little-endian: byte 2 = vertices, byte 3 = faces)
    if 12 * nvox >= 2 ** 31:
        totals = counts.sum(dim=0, dtype=torch.int64).tolist()
        if max(totals) >= 2 ** 31:
            raise L.PscvError(f"{what}: {totals[0]} vertices and {totals[1]} faces do not fit int32 indices")
    vincl = torch.cumsum(counts[:, 0], dim=0, dtype=torch.int32)
    fincl = torch.cumsum(counts[:, 1], dim=0, dtype=torch.int32)
    n_vert, n_face = (int(v) for v in torch.stack((vincl[-1], fincl[-1])).tolist())   # the totals: the one host read
    (xyz, rgb), faces, vkeys = empty(n_vert), torch.empty((n_face, 3), dtype=torch.int32, device=dev), keys(n_vert)
    if n_vert == 0:
        return (xyz, rgb, faces) + vkeys
    rc = _launch("tsdf_brick_emit_vertices", lambda: L.lib().pscv_tsdf_brick_emit_vertices(
        _p(bricks.tsdf_sum), _p(bricks.weight), _p(bricks.rgb_sum), _p(bricks.cweight), _p(info), _p(vincl), *grid, o[0], o[1], o[2], s,
        _p(xyz), _p(rgb), _p(vkeys[0]) if return_keys else None, n_vert, st), cost=lambda: (8.0 * nvox + 60.0 * n_vert, 40.0 * n_vert))
    L.check(rc, "pscv_tsdf_brick_emit_vertices")
    if n_face:
        rc = _launch("tsdf_brick_emit_faces", lambda: L.lib().pscv_tsdf_brick_emit_faces(_p(info), _p(vincl), _p(fincl), *grid, _p(faces),
                                                                                         n_face, st),
                     cost=lambda: (8.0 * nvox + 12.0 * n_face, 0.0))
        L.check(rc, "pscv_tsdf_brick_emit_faces")
    return (xyz, rgb, faces) + vkeys


# --------------------------------------------------------------------------------------------
# mesh clean-up: connected components, fragment removal, vertex normals
# --------------------------------------------------------------------------------------------
MESH_MAX_INDEX = 2 ** 31 - 1


def _mesh_count(value, name, what):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or int(value) < 0:
        raise ValueError(f"{what}: {name} must be an integer >= 0, got {value!r}")
    return int(value)


def _mesh_faces(faces, n_vertices, what):
    """faces int32 [F,3], 0 <= n_vertices < 2^31, 3 F < 2^31 -> (F, V); every complaint is a ValueError."""
    if not torch.is_tensor(faces) or faces.dtype != torch.int32 or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"{what}: faces must be an int32 tensor [F,3], got {getattr(faces, 'dtype', type(faces))} "
                         f"{tuple(getattr(faces, 'shape', ()))}")
    V = _mesh_count(n_vertices, "n_vertices", what)
    F = int(faces.shape[0])
    if V > MESH_MAX_INDEX or 3 * F > MESH_MAX_INDEX:
        raise ValueError(f"{what}: {V} vertices and {F} faces do not fit int32 indices (n_vertices, 3 n_faces < 2^31)")
    return F, V


def _mesh_on_gpu(what, **tensors):
    dev = None
    for name, t in tensors.items():
        if t is None:
            continue
        if not t.is_cuda:
            raise ValueError(f"{what}: {name} must be on the GPU (there is no CPU / PyTorch fallback for the kernels)")
        if not t.is_contiguous():
            raise ValueError(f"{what}: {name} must be contiguous")
        if dev is not None and t.device != dev:
            raise ValueError(f"{what}: {name} is on {t.device}, the other tensors on {dev}")
        dev = t.device


def _mesh_vertices(xyz, rgb, normals, what):
    if not torch.is_tensor(xyz) or xyz.dtype != torch.float32 or xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError(f"{what}: xyz must be an fp32 tensor [V,3], got {getattr(xyz, 'dtype', type(xyz))} {tuple(getattr(xyz, 'shape', ()))}")
    if rgb is not None and (not torch.is_tensor(rgb) or rgb.dtype != torch.uint8 or tuple(rgb.shape) != tuple(xyz.shape)):
        raise ValueError(f"{what}: rgb must be a uint8 tensor {tuple(xyz.shape)}, got {getattr(rgb, 'dtype', type(rgb))} "
                         f"{tuple(getattr(rgb, 'shape', ()))}")
    if normals is not None and (not torch.is_tensor(normals) or normals.dtype != torch.float32 or tuple(normals.shape) != tuple(xyz.shape)):
        raise ValueError(f"{what}: normals must be an fp32 tensor {tuple(xyz.shape)}, got {getattr(normals, 'dtype', type(normals))} "
                         f"{tuple(getattr(normals, 'shape', ()))}")
    return int(xyz.shape[0])


def _mesh_status_error(what, bad_faces, trips):
    if bad_faces:
        return RuntimeError(f"{what}: {bad_faces} faces have an index outside [0, n_vertices)")
    return RuntimeError(f"{what}: {trips} lanes reached the trip limit of the union-find (a defect of the kernel, not of the mesh)")


def _mesh_components(faces, F, V, status):
    """The three launches-worth of pscv_mesh_components and pscv_mesh_component_sizes on the current stream; no host read."""
    dev = faces.device
    label = torch.empty(V, dtype=torch.int32, device=dev)
    fcount = torch.zeros(V, dtype=torch.int32, device=dev)
    vcount = torch.zeros(V, dtype=torch.int32, device=dev)
    if V == 0:
        return label, fcount, vcount
    st = _stream()
    # per face two unions: a few dependent 4-byte atomic reads each and one compare-and-swap (the floor is the atomic rate, not HBM)
    rc = _launch("mesh_components", lambda: L.lib().pscv_mesh_components(_p(faces), F, V, _p(label), _p(status), st),
                 cost=lambda: (12.0 * F + 8.0 * V, 0.0))
    L.check(rc, "pscv_mesh_components")
    rc = _launch("mesh_component_sizes", lambda: L.lib().pscv_mesh_component_sizes(_p(label), _p(faces), F, V, _p(fcount), _p(vcount), st),
                 cost=lambda: (16.0 * F + 4.0 * V, 0.0))
    L.check(rc, "pscv_mesh_component_sizes")
    return label, fcount, vcount


def mesh_components(faces: torch.Tensor, n_vertices: int):
    """Connected components of an indexed triangle mesh on the GPU: faces int32 [F,3] over
    ``n_vertices`` vertices -> (label, fcount, vcount), int32 [n_vertices].  Two vertices are connected when some face contains
    both; ``label[v]`` is the smallest vertex index of v's component (a vertex in no face is its own); ``fcount[r]`` counts the
    faces whose first vertex has label r and ``vcount[r]`` the vertices with label r, both 0 except at roots.  A lock-free
    union-find whose result does not depend on the schedule: bit-reproducible.  One host read (the status words): a face with
    an index outside [0, n_vertices) is a RuntimeError that names how many there are."""
    what = "pscv.mesh_components"
    F, V = _mesh_faces(faces, n_vertices, what)
    _mesh_on_gpu(what, faces=faces)
    status = torch.zeros(2, dtype=torch.int32, device=faces.device)
    out = _mesh_components(faces, F, V, status)
    bad, trips = (F, 0) if V == 0 else status.tolist()
    if bad or trips:
        raise _mesh_status_error(what, bad, trips)
    return out


def mesh_vertex_normals(xyz: torch.Tensor, faces: torch.Tensor) -> torch.Tensor:
    """Area-weighted unit vertex normals of an indexed triangle mesh on the GPU: xyz fp32 [V,3], faces
    int32 [F,3] -> fp32 [V,3].  Per vertex the fp64 sum of (b - a) x (c - a) over the faces that use it, in ascending corner
    order (corner 3 f + k is vertex faces[f,k]; a face that names the vertex twice counts twice), divided by its length and
    rounded to fp32; (0,0,0) for a vertex in no face and when the length is 0 or not finite.  Faces oriented towards free space
    (``tsdf_extract``) give normals that point there.  The vertex -> corner adjacency is a stable torch sort (plumbing); one
    gathering launch, no float atomics, no host read, bit-reproducible.  A face with an index out of range adds nothing."""
    what = "pscv.mesh_vertex_normals"
    V = _mesh_vertices(xyz, None, None, what)
    F, V = _mesh_faces(faces, V, what)
    _mesh_on_gpu(what, xyz=xyz, faces=faces)
    dev = xyz.device
    normals = torch.empty((V, 3), dtype=torch.float32, device=dev)
    if V == 0:
        return normals
    key = faces.reshape(-1).to(torch.int64)
    key = torch.where((key >= 0) & (key < V), key, torch.full_like(key, V))       # (out of range: behind every vertex's corners)
    corners = torch.sort(key, stable=True).indices.to(torch.int32)
    corner_off = torch.zeros(V + 1, dtype=torch.int32, device=dev)
    corner_off[1:] = torch.cumsum(torch.bincount(key, minlength=V + 1)[:V], dim=0)
    rc = _launch("mesh_vertex_normals", lambda: L.lib().pscv_mesh_vertex_normals(_p(xyz), _p(faces), _p(corner_off), _p(corners), F, V,
                                                                                 _p(normals), _stream()),
                 # per corner the face's indices and three positions (48 B, gathered), per vertex its offsets and the normal
                 cost=lambda: (3.0 * F * 52.0 + 20.0 * V, 3.0 * F * 20.0))
    L.check(rc, "pscv_mesh_vertex_normals")
    return normals


def mesh_clean(xyz: torch.Tensor, rgb: torch.Tensor, faces: torch.Tensor, *, min_component_faces: int = 0,
               min_component_fraction: float = 0.0, keep_largest: int = 0, drop_degenerate: bool = False,
               normals: Optional[torch.Tensor] = None):
    """Removes small connected components, degenerate faces and unused vertices from an indexed triangle mesh on the GPU
    (INTEGRATION.md section 2p): xyz fp32 [V,3], rgb uint8 [V,3], faces int32 [F,3] (and ``normals`` fp32 [V,3], carried along)
    -> (xyz, rgb, faces) or (xyz, rgb, faces, normals), vertices and faces in their original relative order, indices renumbered.

    A component (``mesh_components``) survives when it has at least max(``min_component_faces``, ceil(``min_component_fraction``
    x the largest component's faces)) faces, at least one face, and -- with ``keep_largest`` = k > 0 -- is among the first k in the
    order (faces descending, label ascending).  A face survives when its component does and, with ``drop_degenerate``, it has no
    repeated index and its fp64 cross product is not exactly (0,0,0); a vertex survives when a surviving face uses it.  With the
    defaults the call only drops the vertices no face uses.  Applying it twice changes nothing more (the components are those of
    the INPUT mesh: only ``drop_degenerate`` together with a size option can leave a component that a second call, which counts
    it without its degenerate faces, finds too small).  The choice is torch on the
    device, the prefix sums are ``torch.cumsum``; one host read (the two totals and the status words) sizes the outputs."""
    what = "pscv.mesh_clean"
    V = _mesh_vertices(xyz, rgb, normals, what)
    if rgb is None:
        raise ValueError(f"{what}: rgb must be a uint8 tensor {tuple(xyz.shape)}, got None")
    F, V = _mesh_faces(faces, V, what)
    min_faces = _mesh_count(min_component_faces, "min_component_faces", what)
    k_largest = _mesh_count(keep_largest, "keep_largest", what)
    try:
        fraction = float(min_component_fraction)
    except (TypeError, ValueError):
        fraction = float("nan")
    if not 0.0 <= fraction <= 1.0:
        raise ValueError(f"{what}: min_component_fraction must lie in [0, 1], got {min_component_fraction!r}")
    if not isinstance(drop_degenerate, (bool, np.bool_)):
        raise ValueError(f"{what}: drop_degenerate must be a bool, got {drop_degenerate!r}")
    _mesh_on_gpu(what, xyz=xyz, rgb=rgb, faces=faces, normals=normals)
    dev = xyz.device

    def empty():
        out = (xyz.new_empty((0, 3)), rgb.new_empty((0, 3)), faces.new_empty((0, 3)))
        return out if normals is None else out + (normals.new_empty((0, 3)),)

    if V == 0:
        if F:
            raise _mesh_status_error(what, F, 0)
        return empty()
    status = torch.zeros(2, dtype=torch.int32, device=dev)
    label, fcount, vcount = _mesh_components(faces, F, V, status)
    # the choice, on the device
    threshold = torch.clamp(torch.ceil(fraction * fcount.max().to(torch.float64)), min=float(min_faces))
    keep = (fcount > 0) & (fcount.to(torch.float64) >= threshold)
    if k_largest:
        order = torch.sort(fcount, stable=True, descending=True).indices         # (faces descending, label ascending)
        first = torch.zeros(V, dtype=torch.bool, device=dev)
        first[order[:k_largest]] = True
        keep &= first
    keep_comp = keep.to(torch.uint8)
    fmark = torch.empty(F, dtype=torch.int32, device=dev)
    vmark = torch.zeros(V, dtype=torch.int32, device=dev)
    st = _stream()
    rc = _launch("mesh_mark", lambda: L.lib().pscv_mesh_mark(_p(xyz), _p(faces), _p(label), _p(keep_comp), F, V, int(bool(drop_degenerate)),
                                                             _p(fmark), _p(vmark), st),
                 cost=lambda: (F * (12.0 + 4.0 + 1.0 + 4.0 + 12.0 + (36.0 if drop_degenerate else 0.0)), 20.0 * F))
    L.check(rc, "pscv_mesh_mark")
    fincl = torch.cumsum(fmark, dim=0, dtype=torch.int32)
    vincl = torch.cumsum(vmark, dim=0, dtype=torch.int32)
    # the one host read: the two totals and the status words (no face: status[0], which is 0 then, stands in for the empty sum)
    n_face, n_vert, bad, trips = torch.cat((fincl[-1:] if F else status[:1], vincl[-1:], status)).tolist()
    if bad or trips:
        raise _mesh_status_error(what, bad, trips)
    xyz_out = torch.empty((n_vert, 3), dtype=torch.float32, device=dev)
    rgb_out = torch.empty((n_vert, 3), dtype=torch.uint8, device=dev)
    faces_out = torch.empty((n_face, 3), dtype=torch.int32, device=dev)
    normals_out = None if normals is None else torch.empty((n_vert, 3), dtype=torch.float32, device=dev)
    if n_vert:
        rc = _launch("mesh_compact", lambda: L.lib().pscv_mesh_compact(
            _p(xyz), _p(rgb), _p(normals), _p(faces), _p(fmark), _p(vmark), _p(fincl), _p(vincl), F, V, _p(xyz_out), _p(rgb_out),
            _p(normals_out), _p(faces_out), n_face, n_vert, st),
            cost=lambda: (8.0 * (F + V) + n_face * 36.0 + n_vert * (30.0 + (24.0 if normals is not None else 0.0)), 0.0))
        L.check(rc, "pscv_mesh_compact")
    out = (xyz_out, rgb_out, faces_out)
    return out if normals is None else out + (normals_out,)


# --------------------------------------------------------------------------------------------
# scene set-up from a COLMAP sparse model (utils/colmap_utils.py: compute_src_imgs, compute_min_max_depth_yao)
# --------------------------------------------------------------------------------------------
def _sparse_inputs(what, xyz, R, t, **index_arrays):
    """The shared checks of the two sparse-model ops: xyz fp64 [P,3], R fp32 [N,3,3], t fp32 [N,3] or [N,3,1], the named index
    tensors (name -> (tensor, dtype)) one-dimensional, everything contiguous on one HIP device.  -> (t as [N,3], P, N)."""
    tensors = [xyz, R, t] + [v[0] for v in index_arrays.values()]
    _dev(*tensors)
    if xyz.dtype != torch.float64 or xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError(f"{what}: xyz fp64 [P,3] expected, got {xyz.dtype} {tuple(xyz.shape)}")
    if R.dtype != torch.float32 or R.dim() != 3 or tuple(R.shape[1:]) != (3, 3) or R.shape[0] < 1:
        raise ValueError(f"{what}: R fp32 [N,3,3] expected, got {R.dtype} {tuple(R.shape)}")
    n = int(R.shape[0])
    if t.dtype != torch.float32 or tuple(t.shape) not in ((n, 3), (n, 3, 1)):
        raise ValueError(f"{what}: t fp32 [{n},3] (or [{n},3,1]) expected, got {t.dtype} {tuple(t.shape)}")
    for name, (x, dtype) in index_arrays.items():
        if x.dtype != dtype or x.dim() != 1:
            raise ValueError(f"{what}: {name} must be a one-dimensional {dtype} tensor, got {x.dtype} {tuple(x.shape)}")
    if any(x.device != xyz.device for x in tensors):
        raise ValueError(f"{what}: all tensors must be on the same device")
    return t.reshape(n, 3), int(xyz.shape[0]), n


def _in_range(what, name, x, hi):
    """Raise unless every index of ``x`` is in [0, hi): one host read per call; the kernels skip such entries, never follow them."""
    if x.numel() and bool(((x < 0) | (x >= hi)).any()):
        raise ValueError(f"{what}: {name} holds an index outside [0,{hi})")


def sparse_pair_counts(xyz: torch.Tensor, track_off: torch.Tensor, track_img: torch.Tensor, R: torch.Tensor, t: torch.Tensor,
                       min_triangulation_angle: float):
    """The two matrices behind the reference's source-view selection (utils/colmap_utils.py:compute_src_imgs; INTEGRATION.md
    section 2i): xyz fp64 [P,3]; the tracks in CSR form, track_off int64 [P+1] and track_img int32 [nnz] of IMAGE INDICES, sorted
    and without duplicates per point; R fp32 [N,3,3], t fp32 [N,3] (or [N,3,1]), all on the GPU -> (adj, adj_tri) int32 [N,N] on
    the GPU.  ``adj[i,j]`` counts the points images i and j both observe (the diagonal: the points of image i); ``adj_tri[i,j]``
    those whose reference angle for the ordered pair exceeds ``min_triangulation_angle`` degrees (diagonal 0).  One
    pscv_sparse_pair_counts call on the current stream; integer atomics, bit-reproducible.  The index checks before the launch
    read a few flags back to the host (this is a once-per-scene step, not a hot path)."""
    what = "pscv.sparse_pair_counts"
    t, npts, n = _sparse_inputs(what, xyz, R, t, track_off=(track_off, torch.int64), track_img=(track_img, torch.int32))
    nnz = int(track_img.numel())
    if track_off.numel() != npts + 1:
        raise ValueError(f"{what}: track_off must have P + 1 = {npts + 1} entries, got {track_off.numel()}")
    if not float(min_triangulation_angle) >= 0.0:
        raise ValueError(f"{what}: min_triangulation_angle={min_triangulation_angle} must be >= 0")
    _in_range(what, "track_img", track_img, n)
    if bool((track_off[1:] < track_off[:-1]).any()) or int(track_off[0]) != 0 or int(track_off[-1]) != nnz:
        raise ValueError(f"{what}: track_off must rise from 0 to nnz = {nnz}")
    adj = torch.empty((n, n), dtype=torch.int32, device=xyz.device)
    adj_tri = torch.empty_like(adj)
    rc = _launch("sparse_pair_counts", lambda: L.lib().pscv_sparse_pair_counts(
        _p(xyz), _p(track_off), _p(track_img), npts, nnz, _p(R), _p(t), n, float(min_triangulation_angle), _p(adj), _p(adj_tri),
        _stream()))
    L.check(rc, "pscv_sparse_pair_counts")
    return adj, adj_tri


def sparse_depth_ranges(xyz: torch.Tensor, obs_img: torch.Tensor, obs_pt: torch.Tensor, R: torch.Tensor, t: torch.Tensor,
                        perc=(1, 99)):
    """Per-image depth range of the reference (utils/colmap_utils.py:compute_min_max_depth_yao): xyz
    fp64 [P,3]; one entry per observation, obs_img int32 [M] (image index) and obs_pt int32 [M] (row of xyz), in any order, a
    point as often as the image observes it; R fp32 [N,3,3], t fp32 [N,3] (or [N,3,1]), all on the GPU -> (depth_min, depth_max)
    fp64 [N] on the GPU: the ``perc`` percentiles (numpy's linear interpolation) of the fp32-rounded depths (R x + t).z + 1e-6 of
    each image's observations, 0 and 0 for an image without any.  pscv_sparse_obs_depths, ``torch.sort`` of the 64-bit keys
    (plumbing), pscv_segment_percentiles, on the current stream."""
    what = "pscv.sparse_depth_ranges"
    t, npts, n = _sparse_inputs(what, xyz, R, t, obs_img=(obs_img, torch.int32), obs_pt=(obs_pt, torch.int32))
    m = int(obs_img.numel())
    if obs_pt.numel() != m:
        raise ValueError(f"{what}: obs_img and obs_pt differ in length ({m} and {obs_pt.numel()})")
    q_lo, q_hi = (float(q) / 100.0 for q in perc)
    if not (0.0 <= q_lo <= 1.0 and 0.0 <= q_hi <= 1.0):
        raise ValueError(f"{what}: percentiles {tuple(perc)} outside [0,100]")
    _in_range(what, "obs_img", obs_img, n)
    _in_range(what, "obs_pt", obs_pt, npts)
    keys = torch.empty(m, dtype=torch.int64, device=xyz.device)
    rc = _launch("sparse_obs_depths", lambda: L.lib().pscv_sparse_obs_depths(
        _p(xyz), npts, _p(obs_img), _p(obs_pt), m, _p(R), _p(t), n, _p(keys), _stream()))
    L.check(rc, "pscv_sparse_obs_depths")
    keys = torch.sort(keys).values                 # (image indices are below 2^31: the signed order is the unsigned one)
    seg_off = torch.zeros(n + 1, dtype=torch.int64, device=xyz.device)
    seg_off[1:] = torch.cumsum(torch.bincount(obs_img.long(), minlength=n), 0)
    lo = torch.empty(n, dtype=torch.float64, device=xyz.device)
    hi = torch.empty_like(lo)
    rc = _launch("segment_percentiles", lambda: L.lib().pscv_segment_percentiles(
        _p(keys), m, _p(seg_off), n, q_lo, q_hi, _p(lo), _p(hi), _stream()))
    L.check(rc, "pscv_segment_percentiles")
    return lo, hi


TVD_MAX_TUPLES = 65535      # of one pscv_tuple_visible_depths call (one grid row per tuple); longer lists go in chunks


def tuple_visible_depths(xyz: torch.Tensor, track_off: torch.Tensor, track_img: torch.Tensor, tuples: torch.Tensor, K: torch.Tensor,
                         R: torch.Tensor, t: torch.Tensor, sizes: torch.Tensor):
    """The visible depth range of many image tuples at once (utils/colmap_utils.py:compute_min_max_depth_visible; INTEGRATION.md
    section 2j): xyz fp64 [P,3] and the tracks in CSR form as for ``sparse_pair_counts`` (no image twice in a track); tuples int32
    [T,V] of IMAGE INDICES, distinct within a tuple, 3 <= V <= 32; K fp32 [T,V,3,3] the tuples' own intrinsics; R fp32 [N,3,3], t
    fp32 [N,3] (or [N,3,1]) of all images; sizes fp64 [T,V,2] = (width, height), all on the GPU ->
    (min_d fp64 [T,V], max_d fp64 [T,V], min_row int64 [T,V], max_row int64 [T,V], n_pts int32 [T]) on the GPU.
    A point takes part in a tuple when at least 3 of its images observe it (``n_pts``); per view the smallest and largest depth
    among the points that project inside the image with a positive depth, and the lowest row of ``xyz`` that attains each; NaN
    and -1 for a view without such a point.  One pscv_tuple_visible_depths call per 65535 tuples on the current stream;
    bit-reproducible.  The index checks read a few flags back to the host, and the call itself reads the tuples back once."""
    what = "pscv.tuple_visible_depths"
    t, npts, n = _sparse_inputs(what, xyz, R, t, track_off=(track_off, torch.int64), track_img=(track_img, torch.int32))
    _dev(tuples, K, sizes)
    if tuples.dtype != torch.int32 or tuples.dim() != 2 or tuples.shape[0] < 1:
        raise ValueError(f"{what}: tuples int32 [T,V] with T >= 1 expected, got {tuples.dtype} {tuple(tuples.shape)}")
    T, V = int(tuples.shape[0]), int(tuples.shape[1])
    if not 3 <= V <= 32:
        raise ValueError(f"{what}: V={V} outside [3,32]")
    if K.dtype != torch.float32 or tuple(K.shape) != (T, V, 3, 3):
        raise ValueError(f"{what}: K fp32 [{T},{V},3,3] expected, got {K.dtype} {tuple(K.shape)}")
    if sizes.dtype != torch.float64 or tuple(sizes.shape) != (T, V, 2):
        raise ValueError(f"{what}: sizes fp64 [{T},{V},2] expected, got {sizes.dtype} {tuple(sizes.shape)}")
    if any(x.device != xyz.device for x in (tuples, K, sizes)):
        raise ValueError(f"{what}: all tensors must be on the same device")
    if n > 46340:
        raise ValueError(f"{what}: {n} images, more than 46340")
    nnz = int(track_img.numel())
    if track_off.numel() != npts + 1:
        raise ValueError(f"{what}: track_off must have P + 1 = {npts + 1} entries, got {track_off.numel()}")
    _in_range(what, "track_img", track_img, n)
    _in_range(what, "tuples", tuples, n)
    if bool((track_off[1:] < track_off[:-1]).any()) or int(track_off[0]) != 0 or int(track_off[-1]) != nnz:
        raise ValueError(f"{what}: track_off must rise from 0 to nnz = {nnz}")
    ordered = torch.sort(tuples, dim=1).values
    if bool((ordered[:, 1:] == ordered[:, :-1]).any()):
        raise ValueError(f"{what}: a tuple names an image twice")
    dev = xyz.device
    min_d = torch.empty((T, V), dtype=torch.float64, device=dev)
    max_d = torch.empty_like(min_d)
    min_row = torch.empty((T, V), dtype=torch.int64, device=dev)
    max_row = torch.empty_like(min_row)
    n_pts = torch.empty(T, dtype=torch.int32, device=dev)
    for k0 in range(0, T, TVD_MAX_TUPLES):
        k1 = min(T, k0 + TVD_MAX_TUPLES)
        ws = torch.zeros(max(int(L.lib().pscv_tuple_visible_depths_workspace(k1 - k0, V)), 1), dtype=torch.uint8, device=dev)
        rc = _launch("tuple_visible_depths", lambda: L.lib().pscv_tuple_visible_depths(
            _p(xyz), _p(track_off), _p(track_img), npts, nnz, _p(tuples[k0:k1]), _p(K[k0:k1]), _p(R), _p(t), _p(sizes[k0:k1]), n,
            k1 - k0, V, _p(min_d[k0:k1]), _p(max_d[k0:k1]), _p(min_row[k0:k1]), _p(max_row[k0:k1]), _p(n_pts[k0:k1]), _p(ws),
            _stream()),
            # per (tuple, observation) one LDS mask read, twice (the two passes)
            cost=lambda: (float(2 * (k1 - k0) * (nnz * 4 + npts * 16)), 0.0))
        L.check(rc, "pscv_tuple_visible_depths")
    return min_d, max_d, min_row, max_row, n_pts


# --------------------------------------------------------------------------------------------
# image preparation (preprocess.py:157-164, data/MVSDataset.py:read_img, data/md_yao.py:99-102: PIL's Lanczos resize, nearest depth)
# --------------------------------------------------------------------------------------------
LANCZOS_PRECISION_BITS = 32 - 8 - 2      # PIL's fixed point for 8-bit images


@functools.lru_cache(maxsize=256)
def lanczos_tables(in_len: int, out_len: int):
    """PIL's resampling tables of one axis for ``Image.LANCZOS`` on 8-bit images -> (coeff int32
    [out_len, ksize], bounds int32 [out_len, 2] = (first, n), ksize): output sample o reads source samples first .. first + n - 1
    with the 22-bit fixed-point weights coeff[o, :n] (zero past n).  Host code in float64, PIL's operations in PIL's order, whole
    tables at a time except the sines: those are ``math.sin`` (libm, as PIL; numpy's vectorised sine may differ in the last bit).
    Cached per (in_len, out_len); the arrays are read-only."""
    in_len, out_len = int(in_len), int(out_len)
    if in_len < 1 or out_len < 1:
        raise ValueError(f"pscv.lanczos_tables: lengths {in_len} -> {out_len} must be >= 1")
    scale = in_len / out_len
    fs = max(scale, 1.0)
    support = 3.0 * fs
    ksize = 2 * int(math.ceil(support)) + 1
    inv_fs = 1.0 / fs                                     # PIL multiplies by the reciprocal
    center = (np.arange(out_len) + 0.5) * scale
    first = np.maximum((center - support + 0.5).astype(np.int64), 0)              # (a C cast: truncation)
    n = np.minimum((center + support + 0.5).astype(np.int64), in_len) - first
    k = np.arange(ksize, dtype=np.int64)
    x = ((k[None, :] + first[:, None]) - center[:, None] + 0.5) * inv_fs
    live = (k[None, :] < n[:, None]) & (x >= -3.0) & (x < 3.0) & (x != 0.0)      # L(x) = sinc(x) sinc(x / 3) there, 1 at 0, else 0
    a, b = x[live] * math.pi, x[live] / 3 * math.pi
    w = np.where((k[None, :] < n[:, None]) & (x == 0.0), 1.0, 0.0)
    w[live] = (np.array([math.sin(v) for v in a.tolist()]) / a) * (np.array([math.sin(v) for v in b.tolist()]) / b)
    total = np.zeros(out_len)
    for j in range(ksize):                                # in index order, as PIL sums (the zeros past n change nothing)
        total += w[:, j]
    w = np.where(total[:, None] != 0.0, w / np.where(total != 0.0, total, 1.0)[:, None], w)
    one = float(1 << LANCZOS_PRECISION_BITS)
    coeff = np.where(w < 0, np.trunc(-0.5 + w * one), np.trunc(0.5 + w * one)).astype(np.int32)
    bounds = np.stack([first, n], axis=1).astype(np.int32)
    coeff.setflags(write=False)
    bounds.setflags(write=False)
    return coeff, bounds, ksize


_LANCZOS_DEVICE_TABLES = 64      # device copies kept, least recently used first out
_lanczos_device = collections.OrderedDict()
_u8_to_unit = {}


def _lanczos_device_tables(in_len, out_len, axis, device):
    """(coeff, bounds, ksize) on ``device``; the horizontal pass (axis 0) reads its weights transposed, [ksize, out_len]."""
    key = (in_len, out_len, axis, device)
    hit = _lanczos_device.get(key)
    if hit is None:
        coeff, bounds, ksize = lanczos_tables(in_len, out_len)
        coeff = np.ascontiguousarray(coeff.T) if axis == 0 else coeff
        hit = (torch.from_numpy(coeff.copy()).to(device), torch.from_numpy(bounds.copy()).to(device), ksize)
        _lanczos_device[key] = hit
        if len(_lanczos_device) > _LANCZOS_DEVICE_TABLES:
            _lanczos_device.popitem(last=False)
    else:
        _lanczos_device.move_to_end(key)
    return hit


def _unit_table(device):
    """fp32 [256] = numpy's float32(v) / float32(255) on ``device``: the values ``np.array(img, dtype=np.float32) / 255.`` holds."""
    t = _u8_to_unit.get(device)
    if t is None:
        t = _u8_to_unit[device] = torch.from_numpy(np.arange(256, dtype=np.float32) / np.float32(255)).to(device)
    return t


def _resample_pass(src, pitch, lines, in_len, C, axis, tables, out_len, out_first, out_count, dst, dst_f32, lut):
    coeff, bounds, ksize = tables if tables is not None else (None, None, 0)
    rc = _launch("resample_u8_pass", lambda: L.lib().pscv_resample_u8_pass(
        src, pitch, lines, in_len, C, axis, _p(coeff), _p(bounds), ksize, out_len, out_first, out_count, _p(dst), _p(dst_f32), _p(lut),
        _stream()),
        cost=lambda: (float(out_count * lines * C * (ksize + 1 + (4 if dst_f32 is not None else 0))), 0.0))
    L.check(rc, "pscv_resample_u8_pass")


def resize_lanczos_u8(img: torch.Tensor, size, crop=None, want_f32: bool = False):
    """``PIL.Image.resize(size, resample=Image.LANCZOS)`` of an 8-bit image on the GPU, byte for byte.
    img uint8 [H,W,3], [H,W,1] or [H,W] on the GPU, contiguous; ``size`` = (width, height) as PIL takes it; ``crop`` = (x0, y0, w,
    h) in pixels of the resized image: only that window is computed and returned.  -> uint8 [h,w,C] ([h,w] for a [H,W] input);
    with ``want_f32`` also fp32 [C,h,w] = float32(v) / float32(255), the network's input layout.
    At most two pscv_resample_u8_pass launches on the current stream, in PIL's order: the horizontal pass (the window's columns,
    into an 8-bit intermediate) when the width changes, then the vertical pass (the window's rows) when the height changes; an
    image whose size does not change takes the identity pass, which crops and converts."""
    what = "pscv.resize_lanczos_u8"
    _dev(img)
    if img.dtype != torch.uint8:
        raise ValueError(f"{what}: uint8 image expected, got {img.dtype}")
    if img.dim() not in (2, 3) or (img.dim() == 3 and img.shape[2] not in (1, 3)) or img.shape[0] < 1 or img.shape[1] < 1:
        raise ValueError(f"{what}: [H,W,3], [H,W,1] or [H,W] expected, got {tuple(img.shape)}")
    H, W = int(img.shape[0]), int(img.shape[1])
    C = 1 if img.dim() == 2 else int(img.shape[2])
    w, h = (int(v) for v in size)
    if w < 1 or h < 1:
        raise ValueError(f"{what}: size {(w, h)} below 1")
    x0, y0, cw, ch = (0, 0, w, h) if crop is None else (int(v) for v in crop)
    if x0 < 0 or y0 < 0 or cw < 1 or ch < 1 or x0 + cw > w or y0 + ch > h:
        raise ValueError(f"{what}: crop {(x0, y0, cw, ch)} outside the {w} x {h} output")
    dev = img.device
    lut = _unit_table(dev) if want_f32 else None
    out = torch.empty((ch, cw, C), dtype=torch.uint8, device=dev)
    out_f32 = torch.empty((C, ch, cw), dtype=torch.float32, device=dev) if want_f32 else None
    tv = _lanczos_device_tables(H, h, 1, dev) if h != H else None
    src, pitch = img.data_ptr(), W * C
    if w != W:
        th = _lanczos_device_tables(W, w, 0, dev)
        if tv is None:                                     # the rows are kept: the window's rows of the horizontal pass are the result
            _resample_pass(src + y0 * pitch, pitch, ch, W, C, 0, th, w, x0, cw, out, out_f32, lut)
            return _resize_result(img, out, out_f32, want_f32)
        # every source row, the window's columns (which rows the window needs is the vertical table's business)
        tmp = torch.empty((H, cw, C), dtype=torch.uint8, device=dev)
        _resample_pass(src, pitch, H, W, C, 0, th, w, x0, cw, tmp, None, None)
        src, pitch = tmp.data_ptr(), cw * C
    else:
        src += x0 * C                                      # a column window of the source: a pointer and the source's pitch
    # (tmp is freed when this returns; the caching allocator reuses it in stream order, behind the launch below)
    _resample_pass(src, pitch, cw, H, C, 1, tv, h, y0, ch, out, out_f32, lut)
    return _resize_result(img, out, out_f32, want_f32)


def _resize_result(img, out, out_f32, want_f32):
    out = out[:, :, 0] if img.dim() == 2 else out
    return (out, out_f32) if want_f32 else out


def depth_nearest_crop(depth: torch.Tensor, size, crop=None, min_d: float = 0.0, max_d: float = float("inf")):
    """The ground-truth depth of a training view (data/md_yao.py:99-102,123): depth fp32 [th,tw] on the GPU resized to ``size`` =
    (height, width) by ``F.interpolate(mode="nearest")``'s index rule on CPU torch, of which the window ``crop`` = (y0, x0, h, w)
    is kept -> (depth fp32 [h,w], mask uint8 [h,w] = (depth >= min_d) & (depth < max_d), the bounds rounded to fp32 as torch
    compares an fp32 tensor with a number).  One pscv_depth_nearest_crop launch on the current stream."""
    what = "pscv.depth_nearest_crop"
    _dev(depth)
    if depth.dtype != torch.float32 or depth.dim() != 2 or depth.shape[0] < 1 or depth.shape[1] < 1:
        raise ValueError(f"{what}: depth fp32 [th,tw] expected, got {depth.dtype} {tuple(depth.shape)}")
    oh, ow = (int(v) for v in size)
    if oh < 1 or ow < 1:
        raise ValueError(f"{what}: size {(oh, ow)} below 1")
    y0, x0, ch, cw = (0, 0, oh, ow) if crop is None else (int(v) for v in crop)
    if y0 < 0 or x0 < 0 or ch < 1 or cw < 1 or y0 + ch > oh or x0 + cw > ow:
        raise ValueError(f"{what}: crop {(y0, x0, ch, cw)} outside the {oh} x {ow} map")
    out = torch.empty((ch, cw), dtype=torch.float32, device=depth.device)
    mask = torch.empty((ch, cw), dtype=torch.uint8, device=depth.device)
    rc = _launch("depth_nearest_crop", lambda: L.lib().pscv_depth_nearest_crop(
        _p(depth), int(depth.shape[0]), int(depth.shape[1]), oh, ow, y0, x0, ch, cw, float(min_d), float(max_d), _p(out), _p(mask),
        _stream()))
    L.check(rc, "pscv_depth_nearest_crop")
    return out, mask


# --------------------------------------------------------------------------------------------
# training-view augmentation (data/MVSDataset.py:124-150: ColorJitter's brightness and contrast on the PIL image, motion_blur)
# --------------------------------------------------------------------------------------------
AUG_OPS = {"brightness": L.AUG_BRIGHTNESS, "contrast": L.AUG_CONTRAST}
AUG_NO_BLUR = (0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0)


def _augment_record(what, v, rec):
    """One view's record -> ([op, op], [factor, factor], [9 weights]).  ``rec`` is None (nothing happens to the view), a pair
    (steps, kernel) or an object whose ``record()`` returns one: steps = up to two (name, factor) in the order they run, names
    "brightness" / "contrast"; kernel = 3 x 3 numbers or None (no blur)."""
    steps, kernel = ((), None) if rec is None else (rec.record() if hasattr(rec, "record") else rec)
    steps = list(steps)
    if len(steps) > 2:
        raise ValueError(f"{what}: view {v}: {len(steps)} colour steps, at most two")
    ops_v, fac_v = [L.AUG_NONE, L.AUG_NONE], [1.0, 1.0]
    for s, (name, factor) in enumerate(steps):
        if name not in AUG_OPS:
            raise ValueError(f"{what}: view {v}: step '{name}' must be one of {tuple(AUG_OPS)}")
        if AUG_OPS[name] in ops_v:
            raise ValueError(f"{what}: view {v}: '{name}' listed twice")
        factor = float(np.float32(factor))
        if not math.isfinite(factor):
            raise ValueError(f"{what}: view {v}: the factor of '{name}' is not finite")
        ops_v[s], fac_v[s] = AUG_OPS[name], factor
    w = np.asarray(AUG_NO_BLUR if kernel is None else kernel, dtype=np.float32).reshape(-1)
    if w.size != 9 or not np.isfinite(w).all():
        raise ValueError(f"{what}: view {v}: the blur kernel must be 3 x 3 finite numbers")
    return ops_v, fac_v, w.tolist()


def augment_views(imgs_u8: torch.Tensor, params, crop=None) -> torch.Tensor:
    """The reference's ``data_augmentation`` of V views of one size on the GPU: per view up to two
    colour steps -- PIL's ``ImageEnhance.Brightness`` / ``Contrast``, byte for byte -- and a 3 x 3 blur of the fp32 image under
    BORDER_REFLECT_101.  imgs_u8 uint8 [V,H,W,3] on the GPU, contiguous; ``params`` one record per view (see ``_augment_record``;
    ``data.views.ViewAugmentation`` is one); ``crop`` = (x0, y0, w, h): only that window is computed, while contrast's mean and
    the blur's borders stay those of the whole image.  -> fp32 [V,3,h,w].
    Two launches on the current stream (pscv_augment_grey_sums, skipped when no view has a contrast step; pscv_augment_apply), no
    host wait."""
    what = "pscv.augment_views"
    if not isinstance(imgs_u8, torch.Tensor):
        raise ValueError(f"{what}: a uint8 [V,H,W,3] tensor expected, got {type(imgs_u8).__name__}")
    if imgs_u8.dtype != torch.uint8:
        raise ValueError(f"{what}: uint8 images expected, got {imgs_u8.dtype}")
    if imgs_u8.dim() != 4 or imgs_u8.shape[3] != 3 or min(imgs_u8.shape[:3]) < 1:
        raise ValueError(f"{what}: [V,H,W,3] expected, got {tuple(imgs_u8.shape)}")
    if not imgs_u8.is_contiguous():
        raise ValueError(f"{what}: the images must be contiguous")
    V, H, W = (int(v) for v in imgs_u8.shape[:3])
    if V > L.AUG_MAX_VIEWS:
        raise ValueError(f"{what}: {V} views, at most {L.AUG_MAX_VIEWS} in one call")
    params = list(params)
    if len(params) != V:
        raise ValueError(f"{what}: {len(params)} records for {V} views")
    x0, y0, cw, ch = (0, 0, W, H) if crop is None else (int(v) for v in crop)
    if x0 < 0 or y0 < 0 or cw < 1 or ch < 1 or x0 + cw > W or y0 + ch > H:
        raise ValueError(f"{what}: crop {(x0, y0, cw, ch)} outside the {W} x {H} image")
    if not imgs_u8.is_cuda:
        raise ValueError(f"{what}: the images must be on the GPU (there is no CPU path)")
    ops_l, fac_l, w_l = [], [], []
    for v, rec in enumerate(params):
        o, f, w = _augment_record(what, v, rec)
        ops_l += o
        fac_l += f
        w_l += w
    c_ops, c_fac, c_w = (C.c_int * (2 * V))(*ops_l), (C.c_float * (2 * V))(*fac_l), (C.c_float * (9 * V))(*w_l)
    dev = imgs_u8.device
    out = torch.empty((V, 3, ch, cw), dtype=torch.float32, device=dev)
    ws = None
    if L.AUG_CONTRAST in ops_l:
        nbytes = L.lib().pscv_augment_workspace(V)
        L.check(0 if nbytes >= 0 else -1, "pscv_augment_workspace")
        ws = torch.empty(((nbytes + 7) // 8,), dtype=torch.int64, device=dev)
        rc = _launch("augment_grey_sums", lambda: L.lib().pscv_augment_grey_sums(_p(imgs_u8), V, H, W, c_ops, c_fac, _p(ws), _stream()),
                     cost=lambda: (float(V * H * W * 3), 0.0))
        L.check(rc, "pscv_augment_grey_sums")
    rc = _launch("augment_apply", lambda: L.lib().pscv_augment_apply(_p(imgs_u8), V, H, W, c_ops, c_fac, c_w, _p(ws), x0, y0, cw, ch,
                                                                    _p(_unit_table(dev)), _p(out), _stream()),
                 cost=lambda: (float(V * ch * cw * 15), 0.0))
    L.check(rc, "pscv_augment_apply")
    return out


# --------------------------------------------------------------------------------------------
# PatchMatch multi-view stereo (the COLMAP baseline: utils/colmap_utils.py:depthmap_colmap)
# --------------------------------------------------------------------------------------------
PM_DELTA0, PM_THETA0_DEG = 0.25, 30.0      # candidate 9: inverse-depth fraction and normal angle, halved every iteration


def patch_match_schedule(t: int):
    """(delta_t, theta_t) of pass-local iteration t: delta_t = 0.25 / 2^t of the inverse-depth range,
    theta_t = 30 deg / 2^t."""
    return PM_DELTA0 * 0.5 ** t, math.radians(PM_THETA0_DEG) * 0.5 ** t


def _u32(x: int) -> int:
    """A 32-bit unsigned word as the C ABI's int."""
    return C.c_int(int(x) & 0xFFFFFFFF).value


class _PmInputs:
    """Validated device inputs of one reference view: grey images, camera blocks, pointer arrays, limits."""

    def __init__(self, ref, srcs, cams, src_depths, radius, step, top_k, depth_range=None, what="pscv.patch_match"):
        srcs = list(srcs)
        S = len(srcs)
        if not 1 <= S <= L.PM_MAX_SRC:
            raise ValueError(f"{what}: 1..{L.PM_MAX_SRC} source views expected (PSCV_PM_MAX_SRC), got {S}")
        if not 1 <= int(radius) <= L.PM_MAX_RADIUS:
            raise ValueError(f"{what}: window radius {radius} outside [1,{L.PM_MAX_RADIUS}] (the LDS tile's halo)")
        if not 1 <= int(step) <= int(radius):
            raise ValueError(f"{what}: window step {step} outside [1,radius={radius}]")
        top_k = min(S, 3) if top_k is None else int(top_k)
        if not 1 <= top_k <= min(S, L.PM_MAX_TOPK):
            raise ValueError(f"{what}: top_k={top_k} outside [1,min(S={S},{L.PM_MAX_TOPK})]")
        if depth_range is not None:
            dmin, dmax = (float(np.float32(x)) for x in depth_range)
            if not 0.0 < dmin < dmax or not math.isfinite(dmax):
                raise ValueError(f"{what}: need 0 < depth_min < depth_max, got {depth_range}")
        _dev(ref, cams)
        srcs, self.sptr, self.hw = _maps(srcs, what)
        if ref.dtype != torch.float32 or ref.dim() != 2:
            raise ValueError(f"{what}: the reference must be a fp32 [h,w] grey image, got {ref.dtype} {tuple(ref.shape)}")
        _check_cams(cams, S + 1, what)
        self.ref, self.srcs, self.cams = ref, srcs, cams
        self.h, self.w = ref.shape
        self.S, self.radius, self.step, self.top_k = S, int(radius), int(step), top_k
        self.dptr = None
        self.src_depths = None
        if src_depths is not None:
            src_depths = list(src_depths)
            if len(src_depths) != S:
                raise ValueError(f"{what}: {S} source depth maps expected, got {len(src_depths)}")
            self.src_depths, self.dptr, _ = _maps(src_depths, what)
            if any(d.shape != s.shape for s, d in zip(srcs, src_depths)):
                raise ValueError(f"{what}: source depth maps must be fp32 of their image's size")

    def check_state(self, state, what):
        _dev(state)
        if state.dtype != torch.float32 or tuple(state.shape) != (self.h, self.w, 4):
            raise ValueError(f"{what}: state must be fp32 [h,w,4] = (depth, normal), got {state.dtype} {tuple(state.shape)}")

    def taps(self):
        return (2 * (self.radius // self.step) + 1) ** 2


def patch_match_init(h: int, w: int, cams: torch.Tensor, depth_min: float, depth_max: float, *, seed: int = 0,
                     view: int = 0) -> torch.Tensor:
    """Random initial state fp32 [h,w,4] (candidate 10 of section 2h at every pixel); cams row 0 = the reference view."""
    if not 0.0 < float(np.float32(depth_min)) < float(np.float32(depth_max)):
        raise ValueError(f"pscv.patch_match_init: need 0 < depth_min < depth_max, got {depth_min}, {depth_max}")
    _dev(cams)
    _check_cams(cams, None, "pscv.patch_match_init")
    state = torch.empty((int(h), int(w), 4), dtype=torch.float32, device=cams.device)
    rc = _launch("patch_match_init", lambda: L.lib().pscv_patch_match_init(_p(state), int(h), int(w), _p(cams), float(depth_min),
                                                                          float(depth_max), _u32(seed), _u32(view), _stream()))
    L.check(rc, "pscv_patch_match_init")
    return state


def patch_match_cost(state: torch.Tensor, ref: torch.Tensor, srcs: Sequence[torch.Tensor], cams: torch.Tensor, *,
                     src_depths: Optional[Sequence[torch.Tensor]] = None, radius: int = 5, step: int = 1,
                     top_k: Optional[int] = None):
    """Costs of the hypotheses in ``state`` fp32 [h,w,4] (depth, normal): ref grey fp32 [h,w], srcs S x grey fp32 [h_s,w_s], cams
    [S+1,30] (``geo_filter_cams``, reference first), all on the GPU -> (c_s fp32 [S,h,w] photometric, e_s fp32 [S,h,w] or None
    (with ``src_depths``), aggregated cost fp32 [h,w]: mean of the ``top_k`` (default min(S,3)) smallest c_s, + 0.3 min(e_s, 3)
    in geometric mode).  An invalid source costs exactly 2."""
    x = _PmInputs(ref, srcs, cams, src_depths, radius, step, top_k, what="pscv.patch_match_cost")
    x.check_state(state, "pscv.patch_match_cost")
    cost = torch.empty((x.S, x.h, x.w), dtype=torch.float32, device=ref.device)
    err = torch.empty_like(cost) if src_depths is not None else None
    agg = torch.empty((x.h, x.w), dtype=torch.float32, device=ref.device)
    rc = _launch("patch_match_cost", lambda: L.lib().pscv_patch_match_cost(
        _p(state), _p(ref), x.h, x.w, x.sptr, x.hw, x.S, _p(cams), x.dptr, x.radius, x.step, x.top_k, _p(cost), _p(err), _p(agg),
        _stream()), cost=lambda: (float(x.h * x.w * x.S * x.taps() * 16), float(x.h * x.w * x.S * x.taps() * 30)))
    L.check(rc, "pscv_patch_match_cost")
    return cost, err, agg


def patch_match_half_step(state: torch.Tensor, ref: torch.Tensor, srcs: Sequence[torch.Tensor], cams: torch.Tensor,
                          depth_min: float, depth_max: float, *, colour: int, iteration: int, delta: float, theta: float,
                          seed: int = 0, view: int = 0, src_depths: Optional[Sequence[torch.Tensor]] = None, radius: int = 5,
                          step: int = 1, top_k: Optional[int] = None, want_choice: bool = False, want_candidates: bool = False,
                          _x: Optional[_PmInputs] = None):
    """One red-black half-step of section 2h, in place on ``state`` (the pixels with (row + col) % 2 == colour).  ``iteration`` is
    the 32-bit word the random draws hash; ``delta`` / ``theta`` the perturbation of candidate 9.  Returns (choice int32 [h,w] or
    None, candidates fp32 [h,w,11,4] or None) as asked."""
    x = _x or _PmInputs(ref, srcs, cams, src_depths, radius, step, top_k, (depth_min, depth_max), "pscv.patch_match_half_step")
    if _x is None:
        x.check_state(state, "pscv.patch_match_half_step")
    if colour not in (0, 1):
        raise ValueError(f"pscv.patch_match_half_step: colour {colour} is not 0 or 1")
    choice = torch.full((x.h, x.w), -1, dtype=torch.int32, device=ref.device) if want_choice else None
    cand = torch.zeros((x.h, x.w, 11, 4), dtype=torch.float32, device=ref.device) if want_candidates else None
    rc = _launch("patch_match_half_step", lambda: L.lib().pscv_patch_match_half_step(
        _p(state), _p(ref), x.h, x.w, x.sptr, x.hw, x.S, _p(cams), x.dptr, float(depth_min), float(depth_max), x.radius, x.step,
        x.top_k, _u32(seed), _u32(view), _u32(iteration), int(colour), float(delta), float(theta), _p(choice), _p(cand), _stream()),
        # per pixel of the colour: 11 candidates x S sources x taps bilinear gathers (16 B) and ~30 flops each
        cost=lambda: (float(x.h * x.w // 2 * 11 * x.S * x.taps() * 16), float(x.h * x.w // 2 * 11 * x.S * x.taps() * 30)))
    L.check(rc, "pscv_patch_match_half_step")
    return choice, cand


def patch_match(ref: torch.Tensor, srcs: Sequence[torch.Tensor], cams: torch.Tensor, depth_min: float, depth_max: float, *,
                num_iterations: int = 8, seed: int = 0, view: int = 0, src_depths: Optional[Sequence[torch.Tensor]] = None,
                state: Optional[torch.Tensor] = None, radius: int = 5, step: int = 1, top_k: Optional[int] = None) -> torch.Tensor:
    """PatchMatch stereo of one reference view -> state fp32 [h,w,4] (depth, normal in the reference
    frame).  Photometric pass: from the random initialisation (or ``state``).  Geometric pass (``src_depths``, the sources'
    photometric depth maps): from ``state``, the view's photometric result, with c_s + 0.3 min(e_s, 3).  ``num_iterations`` red +
    black half-steps on the current stream, no host synchronisation; the result is bit-reproducible."""
    pas = 0 if src_depths is None else 1
    x = _PmInputs(ref, srcs, cams, src_depths, radius, step, top_k, (depth_min, depth_max), "pscv.patch_match")
    if int(num_iterations) < 0 or int(num_iterations) > 0xFFFF:
        raise ValueError(f"pscv.patch_match: num_iterations={num_iterations} outside [0,65535]")
    if state is None:
        if pas:
            raise ValueError("pscv.patch_match: the geometric pass starts from the view's photometric state")
        state = patch_match_init(x.h, x.w, cams, depth_min, depth_max, seed=seed, view=view)
    else:
        x.check_state(state, "pscv.patch_match")
        state = state.clone()
    for t in range(int(num_iterations)):
        delta, theta = patch_match_schedule(t)
        for colour in (0, 1):
            patch_match_half_step(state, ref, srcs, cams, depth_min, depth_max, colour=colour, iteration=(pas << 16) | t,
                                  delta=delta, theta=theta, seed=seed, view=view, _x=x)
    return state


def patch_match_filter(state: torch.Tensor, ref: torch.Tensor, srcs: Sequence[torch.Tensor], cams: torch.Tensor,
                       src_depths: Sequence[torch.Tensor], *, radius: int = 5, step: int = 1, want_count: bool = False):
    """COLMAP's filter on ``state`` (section 2h): a pixel is kept when at least 2 sources have c_s <= 0.9, a triangulation angle
    >= 3 deg and e_s <= 1 px against ``src_depths`` -> (depth fp32 [h,w], normal fp32 [h,w,3]), 0 where filtered out (and the
    int32 [h,w] count of passing sources with ``want_count``)."""
    if src_depths is None:
        raise ValueError("pscv.patch_match_filter: the sources' depth maps are required")
    x = _PmInputs(ref, srcs, cams, src_depths, radius, step, 1, what="pscv.patch_match_filter")
    x.check_state(state, "pscv.patch_match_filter")
    depth = torch.empty((x.h, x.w), dtype=torch.float32, device=ref.device)
    normal = torch.empty((x.h, x.w, 3), dtype=torch.float32, device=ref.device)
    count = torch.empty((x.h, x.w), dtype=torch.int32, device=ref.device) if want_count else None
    rc = _launch("patch_match_filter", lambda: L.lib().pscv_patch_match_filter(
        _p(state), _p(ref), x.h, x.w, x.sptr, x.hw, x.S, _p(cams), x.dptr, x.radius, x.step, _p(depth), _p(normal), _p(count),
        _stream()), cost=lambda: (float(x.h * x.w * x.S * x.taps() * 16), float(x.h * x.w * x.S * x.taps() * 30)))
    L.check(rc, "pscv_patch_match_filter")
    return (depth, normal, count) if want_count else (depth, normal)


def grey_image(img: torch.Tensor) -> torch.Tensor:
    """[3,H,W] image in [0,1] -> fp32 grey [H,W] on the same device: x 255 truncated to bytes (the ToPILImage path), then
    (0.299 R + 0.587 G + 0.114 B) / 255 (plumbing, section 2h)."""
    b = torch.floor(img.to(torch.float32) * 255.0).clamp(0, 255)
    return ((0.299 * b[0] + 0.587 * b[1] + 0.114 * b[2]) / 255.0).to(torch.float32).contiguous()


# --------------------------------------------------------------------------------------------
# point-cloud metrics (the step after fusion): grids, bounded nearest neighbour, radius MIS
# --------------------------------------------------------------------------------------------
GRID_SPAN = 1 << 21          # cells per axis a grid can address (21-bit key fields)


@dataclass
class PointGrid:
    """A sparse uniform grid of ``n`` points built by ``point_grid`` (pscv_point_grid_build): ``buf`` is its device buffer,
    ``origin`` / ``cell`` its lattice.  ``occupied()`` reads the number of non-empty cells (synchronises)."""
    buf: torch.Tensor
    n: int
    origin: tuple
    cell: float

    def occupied(self) -> int:
        return int(self.buf[:4].view(torch.int32).item())


def _points(pts: torch.Tensor, what: str) -> torch.Tensor:
    _dev(pts)
    if pts.dtype != torch.float32 or pts.dim() != 2 or pts.shape[1] != 3:
        raise ValueError(f"pscv.{what}: float32 [n,3] points expected, got {pts.dtype} {tuple(pts.shape)}")
    if pts.shape[0] >= (1 << 30):
        raise ValueError(f"pscv.{what}: {pts.shape[0]} points (at most 2^30 - 1)")
    pts = pts.contiguous()
    if pts.numel() and not bool(torch.isfinite(pts).all()):
        raise ValueError(f"pscv.{what}: points must be finite")
    return pts


def _extent(*clouds: torch.Tensor):
    """(min xyz, max xyz) in fp64 over the non-empty clouds, or None."""
    ne = [c for c in clouds if c.shape[0]]
    if not ne:
        return None
    lo = torch.stack([c.amin(0) for c in ne]).amin(0).double().cpu().numpy()
    hi = torch.stack([c.amax(0) for c in ne]).amax(0).double().cpu().numpy()
    return lo, hi


def point_grid(pts: torch.Tensor, cell: float, origin=None, payload: Optional[torch.Tensor] = None) -> PointGrid:
    """Sparse uniform grid of float32 [n,3] points on the GPU (pscv_point_grid_build: hash table of cell keys, counts, scan,
    scatter; no sort and nothing dense over the bounding box).  ``origin`` defaults to the points' minimum corner less one cell;
    every point must lie within 2^21 cells of it.  ``payload`` (int32 [n]) is carried into slot order."""
    pts = _points(pts, "point_grid")
    n = int(pts.shape[0])
    cell = float(cell)
    if not (cell > 0.0 and np.isfinite(cell)):
        raise ValueError(f"pscv.point_grid: cell edge {cell} must be positive and finite")
    ext = _extent(pts)
    if origin is None:
        origin = (0.0, 0.0, 0.0) if ext is None else tuple(float(v) - cell for v in ext[0])
    origin = tuple(float(v) for v in origin)
    if ext is not None:
        lo = (ext[0] - np.array(origin)) / cell
        hi = (ext[1] - np.array(origin)) / cell
        if lo.min() < 0.0 or hi.max() >= GRID_SPAN - 2:
            raise ValueError(f"pscv.point_grid: the points span cells {lo.min():.0f}..{hi.max():.0f} of the origin; at most 0..{GRID_SPAN - 3}")
    if payload is not None:
        _dev(payload)
        if payload.dtype != torch.int32 or tuple(payload.shape) != (n,):
            raise ValueError("pscv.point_grid: payload must be int32 [n]")
        payload = payload.contiguous()
    nbytes = int(L.lib().pscv_point_grid_workspace(n))
    buf = torch.empty(nbytes, dtype=torch.uint8, device=pts.device)
    rc = _launch("point_grid_build", lambda: L.lib().pscv_point_grid_build(
        _p(pts), n, origin[0], origin[1], origin[2], cell, _p(payload), _p(buf), nbytes, _stream()),
        cost=lambda: (float(n * 40), float(n * 20)))
    L.check(rc, "pscv_point_grid_build")
    return PointGrid(buf, n, origin, cell)


def radius_downsample(pts: torch.Tensor, dst: float, rank: torch.Tensor, *, check_every: int = 4):
    """Greedy maximal independent set of the radius graph (|p - q| <= dst in fp64) in ``rank`` order -- what the reference's
    ``metrics.reduce_pts`` computes with rank = the inverse of its random permutation.
    pts float32 [n,3], rank int32 [n] (a permutation of 0..n-1; lower goes first), both on the GPU -> (kept points float32 [k,3],
    mask bool [n] in the input order, number of rounds).  Rounds of pscv_radius_mis_round run on the current stream; the host
    reads the undecided count once every ``check_every`` rounds."""
    pts = _points(pts, "radius_downsample")
    n = int(pts.shape[0])
    _dev(rank)
    dst = float(dst)
    if not (dst >= 0.0 and np.isfinite(dst)):
        raise ValueError(f"pscv.radius_downsample: dst {dst} must be >= 0 and finite")
    rank = rank.to(torch.int32).contiguous()
    if tuple(rank.shape) != (n,):
        raise ValueError(f"pscv.radius_downsample: rank must be [n] = [{n}], got {tuple(rank.shape)}")
    dev = pts.device
    if n == 0:
        return pts[:0], torch.zeros(0, dtype=torch.bool, device=dev), 0
    if int(rank.min()) != 0 or int(rank.max()) != n - 1 or not bool((torch.bincount(rank, minlength=n) == 1).all()):
        raise ValueError("pscv.radius_downsample: rank must be a permutation of 0..n-1")
    lo, hi = _extent(pts)
    cell = max(dst * (1.0 + 1e-6), float((hi - lo).max() + 1e-6) / (GRID_SPAN - 8))     # >= dst: 27 cells hold a neighbourhood
    grid = point_grid(pts, cell, payload=rank)
    state = [torch.zeros(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)]
    k = max(1, int(check_every))
    counters = torch.zeros(k, dtype=torch.int64, device=dev)
    launched = 0
    while True:
        counters.zero_()
        for j in range(k):
            src, nxt, cnt = state[launched % 2], state[(launched + 1) % 2], counters[j:j + 1]
            rc = _launch("radius_mis_round", lambda: L.lib().pscv_radius_mis_round(
                _p(grid.buf), n, grid.origin[0], grid.origin[1], grid.origin[2], grid.cell, dst, _p(src), _p(nxt), _p(cnt), _stream()))
            L.check(rc, "pscv_radius_mis_round")
            launched += 1
        left = counters.cpu().numpy()
        if left[-1] == 0:
            rounds = launched - k + 1 + int(np.argmax(left == 0))     # (the rounds after the first empty one change nothing)
            break
        if launched > n + k:
            raise L.PscvError("pscv.radius_downsample: the rounds do not converge")
    final = state[launched % 2]
    mask = torch.empty(n, dtype=torch.uint8, device=dev)
    kept = torch.empty(n, dtype=torch.int32, device=dev)
    n_kept = torch.empty(1, dtype=torch.int64, device=dev)
    ws_bytes = int(L.lib().pscv_radius_mis_workspace(n))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    rc = _launch("radius_mis_compact", lambda: L.lib().pscv_radius_mis_compact(
        _p(grid.buf), n, _p(final), _p(mask), _p(kept), _p(n_kept), _p(ws), ws_bytes, _stream()))
    L.check(rc, "pscv_radius_mis_compact")
    m = int(n_kept.item())
    return pts.index_select(0, kept[:m].long()), mask.bool(), rounds


def _nn_grids(target: torch.Tensor, maxdist: float, fine_cell: Optional[float], ext):
    """(fine grid, coarse grid) of the targets with one origin: coarse cells of maxdist / 4; fine cells halved from maxdist / 16
    until a non-empty cell holds at most ~12 points on average (or as given)."""
    span = 0.0 if ext is None else float((ext[1] - ext[0]).max())
    floor_cell = (span + 1e-6) / (GRID_SPAN - 8)
    coarse = max(maxdist / 4.0, floor_cell)
    origin = (0.0, 0.0, 0.0) if ext is None else tuple(float(v) - coarse for v in ext[0])
    if fine_cell is not None:
        fine = point_grid(target, max(float(fine_cell), floor_cell), origin)
    else:
        h = max(coarse / 4.0, floor_cell)
        fine = point_grid(target, h, origin)
        for _ in range(8):
            if target.shape[0] == 0 or target.shape[0] <= 12 * fine.occupied() or h / 2.0 < floor_cell:
                break
            h /= 2.0
            fine = point_grid(target, h, origin)
    return fine, point_grid(target, coarse, origin)


def dtu_cells(bb, maxdist: float):
    """Cells per axis of the DTU blocking of ``metrics.chamfer``: floor((bb1 - bb0) / maxdist) + 1."""
    bb = np.asarray(bb, dtype=np.float64).reshape(2, 3)
    return tuple(int(v) + 1 for v in np.floor((bb[1] - bb[0]) / maxdist))


def nn_dist(query: torch.Tensor, target: torch.Tensor, maxdist: float, bb=None, *, fine_cell: Optional[float] = None) -> torch.Tensor:
    """Bounded nearest-neighbour distance: query float32 [m,3], target float32 [n,3] on the GPU ->
    float64 [m]: the distance to the nearest target when it is strictly below ``maxdist``, +inf otherwise (``metrics.chamfer_imw``;
    maxdist = inf is allowed).  ``bb`` ([2,3] fp64, DTU) applies ``metrics.chamfer``'s blocking by cells of ``maxdist``: a query
    in no cell, or whose cell's expanded box holds no target, gets ``maxdist``, and only the targets in that box count."""
    query = _points(query, "nn_dist")
    target = _points(target, "nn_dist")
    maxdist = float(maxdist)
    m, n = int(query.shape[0]), int(target.shape[0])
    dev = query.device
    out = torch.empty(m, dtype=torch.float64, device=dev)
    if not maxdist > 0.0:
        raise ValueError(f"pscv.nn_dist: maxdist {maxdist} must be positive")
    ext_all = _extent(query, target)
    if np.isinf(maxdist):
        if bb is not None:
            raise ValueError("pscv.nn_dist: the DTU mode needs a finite maxdist")
        # no distance between the two clouds reaches their joint bounding-box diagonal: a finite bound with the same results
        maxdist = 1.0 if ext_all is None else float(np.linalg.norm(ext_all[1] - ext_all[0])) * 2.0 + 1.0
    if m == 0:
        return out
    fine, coarse = _nn_grids(target, maxdist, fine_cell, _extent(target))
    coarse_rings = int(np.ceil(maxdist / coarse.cell)) + 1
    bb_arg, occ = None, None
    if bb is not None:
        bbn = np.ascontiguousarray(np.asarray(bb, dtype=np.float64).reshape(2, 3))
        cells = dtu_cells(bbn, maxdist)
        if min(cells) < 1 or max(cells) > 4096:
            raise ValueError(f"pscv.nn_dist: {cells} DTU cells (bb / maxdist)")
        bb_host = (C.c_double * 6)(*bbn.reshape(-1).tolist())
        bb_arg = C.cast(bb_host, C.c_void_p)
        occ = torch.zeros(int(np.prod(cells)), dtype=torch.int32, device=dev)
        rc = _launch("dtu_cell_occupancy", lambda: L.lib().pscv_dtu_cell_occupancy(_p(target), n, bb_arg, maxdist, _p(occ), _stream()))
        L.check(rc, "pscv_dtu_cell_occupancy")
    o = fine.origin
    rc = _launch("point_nn_dist", lambda: L.lib().pscv_point_nn_dist(
        _p(query), m, _p(fine.buf), _p(coarse.buf), n, o[0], o[1], o[2], fine.cell, coarse.cell, 2, coarse_rings, maxdist, bb_arg,
        _p(occ), _p(out), _stream()))
    L.check(rc, "pscv_point_nn_dist")
    return out


# --------------------------------------------------------------------------------------------
# mesh metrics: surface samples proportional to area, bounded distance to the surface
# --------------------------------------------------------------------------------------------
MESH_MAX_SAMPLES = 2 ** 31 - 2
MESH_MAX_PAIRS = 2 ** 31 - 1


def _mesh_spacing(spacing, what):
    try:
        s = float(spacing)
    except (TypeError, ValueError):
        s = float("nan")
    if isinstance(spacing, bool) or not (s > 0.0 and np.isfinite(s) and 0.0 < s * s < float("inf")):
        raise ValueError(f"{what}: spacing must be a positive number with a finite, non-zero square, got {spacing!r}")
    return s


def _mesh_seed(seed, what):
    """Any integer, taken modulo 2^64 -> the signed 64-bit word the C ABI carries it in."""
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)):
        raise ValueError(f"{what}: seed must be an integer, got {seed!r}")
    s = int(seed) & (2 ** 64 - 1)
    return s - 2 ** 64 if s >= 2 ** 63 else s


def _mesh_sample_total(total, spacing, what):
    if total > MESH_MAX_SAMPLES:
        raise ValueError(f"{what}: spacing {spacing} gives {total} samples, more than 2^31 - 2: use a larger spacing")
    return int(total)


def _mesh_pair_total(total, cell, what):
    if total > MESH_MAX_PAIRS:
        raise ValueError(f"{what}: cells of {cell} give {total} (cell, face) pairs, more than 2^31 - 1: use a larger cell")
    return int(total)


def _mesh_cloud_shapes(what, **clouds):
    for name, pts in clouds.items():
        if not torch.is_tensor(pts) or pts.dtype != torch.float32 or pts.dim() != 2 or pts.shape[1] != 3:
            raise ValueError(f"pscv.{what}: {name} must be an fp32 tensor [n,3], got {getattr(pts, 'dtype', type(pts))} "
                             f"{tuple(getattr(pts, 'shape', ()))}")


def _mesh_points(what, **clouds):
    """Finite float32 [n,3] clouds: a host tensor's finiteness is checked here, so that the complaint is a named ValueError that
    needs no device; then the ``_points`` check of each cloud (device, contiguity, finiteness on the device)."""
    for name, pts in clouds.items():
        if not pts.is_cuda and pts.numel() and not bool(torch.isfinite(pts).all()):
            raise ValueError(f"pscv.{what}: {name} must be finite")
    return [_points(pts, what) for pts in clouds.values()]


def mesh_sample(xyz: torch.Tensor, faces: torch.Tensor, spacing: float, *, seed: int = 0, return_faces: bool = False):
    """Deterministic samples of the surface of an indexed triangle mesh, on average one per ``spacing``^2 of area (INTEGRATION.md
    section 2r): xyz fp32 [V,3], faces int32 [F,3] on the GPU -> fp32 [N,3], and with ``return_faces`` the face int32 [N] each
    sample lies on.  Face f gets floor(A_f / spacing^2 + r_f) samples (fp64 area, r_f in [0,1) from a splitmix64 hash of
    (seed, f): stochastic rounding, so faces far smaller than spacing^2 still get their share); a face with zero or non-finite area
    or an index out of range gets none.  The output is face-major; sample k of face f is a + u (b - a) + v (c - a) with (u, v) from
    the hash of (seed, f, k), folded into the triangle.  Integer scan, no float atomics: the same bits on every call.  One host
    read (N); more than 2^31 - 2 samples is a ValueError that names the spacing."""
    what = "pscv.mesh_sample"
    V = _mesh_vertices(xyz, None, None, what)
    F, V = _mesh_faces(faces, V, what)
    spacing = _mesh_spacing(spacing, what)
    seed = _mesh_seed(seed, what)
    _mesh_on_gpu(what, xyz=xyz, faces=faces)
    dev = xyz.device
    lib, st = L.lib(), _stream()
    n = 0
    if F:
        ws_bytes = int(lib.pscv_mesh_scan_workspace(F))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        offsets = torch.empty(F, dtype=torch.int32, device=dev)
        total = torch.empty(1, dtype=torch.int64, device=dev)
        rc = _launch("mesh_sample_count", lambda: lib.pscv_mesh_sample_count(_p(xyz), _p(faces), F, V, spacing, seed, _p(offsets), _p(total),
                                                                             _p(ws), ws_bytes, st),
                     cost=lambda: (F * (12.0 + 36.0 + 12.0), F * 30.0))
        L.check(rc, "pscv_mesh_sample_count")
        n = _mesh_sample_total(int(total.item()), spacing, what)        # the one host read
    out = torch.empty((n, 3), dtype=torch.float32, device=dev)
    face_out = torch.empty(n, dtype=torch.int32, device=dev) if return_faces else None
    if n:
        rc = _launch("mesh_sample_emit", lambda: lib.pscv_mesh_sample_emit(_p(xyz), _p(faces), _p(offsets), F, V, seed, n, _p(out), _p(face_out),
                                                                           st),
                     cost=lambda: (n * (12.0 + 36.0 + 12.0 + (4.0 if return_faces else 0.0)), n * 12.0))
        L.check(rc, "pscv_mesh_sample_emit")
    return (out, face_out) if return_faces else out


@dataclass
class MeshGrid:
    """A sparse uniform grid over the faces of a mesh built by pscv_mesh_grid_build: every face in every cell its bounding box
    touches; ``pairs`` (cell, face) pairs in ``buf``."""
    buf: torch.Tensor
    pairs: int
    origin: tuple
    cell: float


def _mesh_grid(xyz, faces, F, V, origin, cell, what) -> MeshGrid:
    dev = xyz.device
    lib, st = L.lib(), _stream()
    ws_bytes = int(lib.pscv_mesh_scan_workspace(F))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    pair_off = torch.empty(F, dtype=torch.int32, device=dev)
    total = torch.empty(1, dtype=torch.int64, device=dev)
    rc = _launch("mesh_grid_count", lambda: lib.pscv_mesh_grid_count(_p(xyz), _p(faces), F, V, origin[0], origin[1], origin[2], cell,
                                                                     _p(pair_off), _p(total), _p(ws), ws_bytes, st))
    L.check(rc, "pscv_mesh_grid_count")
    pairs = _mesh_pair_total(int(total.item()), cell, what)
    nbytes = int(lib.pscv_mesh_grid_workspace(pairs))
    buf = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    rc = _launch("mesh_grid_build", lambda: lib.pscv_mesh_grid_build(_p(xyz), _p(faces), _p(pair_off), F, V, origin[0], origin[1], origin[2],
                                                                     cell, pairs, _p(buf), nbytes, st))
    L.check(rc, "pscv_mesh_grid_build")
    return MeshGrid(buf, pairs, origin, cell)


def _mesh_cells(xyz, faces, V, maxdist, cell):
    """(origin, fine cell, coarse cell) of the two grids of a mesh: fine cells of twice the mean bounding-box side of the faces (or
    ``cell``), coarse cells of maxdist / 4 and no smaller than the fine ones; both at least the 21-bit span allows."""
    lo, hi = _extent(xyz)
    floor_cell = (float((hi - lo).max()) + 1e-6) / (GRID_SPAN - 8)
    if cell is not None:
        fine = max(float(cell), floor_cell)
    else:
        idx = faces.long()
        tri = xyz[idx[((idx >= 0) & (idx < V)).all(dim=1)]]                  # [valid faces, 3 corners, 3]
        side = float((tri.amax(dim=1) - tri.amin(dim=1)).amax(dim=1).double().mean()) if tri.shape[0] else 0.0
        fine = max(2.0 * side, floor_cell)
    coarse = max(maxdist / 4.0, fine)
    return tuple(float(v) - fine for v in lo), fine, coarse            # (one fine cell of margin: every vertex stays inside the span)


def mesh_dist(query: torch.Tensor, xyz: torch.Tensor, faces: torch.Tensor, maxdist: float, *, return_faces: bool = False,
              cell: Optional[float] = None):
    """Exact bounded distance from points to the surface of an indexed triangle mesh: query fp32 [m,3],
    xyz fp32 [V,3], faces int32 [F,3] on the GPU -> float64 [m]: the distance to the nearest point of any triangle when it is
    strictly below ``maxdist``, +inf otherwise (``nn_dist`` without ``bb``; maxdist = inf is allowed).  With ``return_faces`` also
    int32 [m]: the face that attains the minimum, the lowest index among equals ((d^2, face) compared lexicographically), -1 where
    the distance is inf.  Per face the squared plane distance when the projection falls inside the triangle, otherwise the nearest
    of its three edges, in fp64 from the fp32 coordinates: degenerate faces (a segment, a point) need no special case; a face with
    an index out of range is skipped.  The index is a fine and a coarse uniform grid over the faces (``cell`` overrides the fine
    edge); no result depends on the cell sizes or on the order of the build's atomics.  Queries and vertices must be finite."""
    what = "mesh_dist"
    _mesh_cloud_shapes(what, query=query, xyz=xyz)
    F, V = _mesh_faces(faces, int(xyz.shape[0]), f"pscv.{what}")
    try:
        maxdist = float(maxdist)
    except (TypeError, ValueError):
        maxdist = float("nan")
    if not maxdist > 0.0:
        raise ValueError(f"pscv.{what}: maxdist {maxdist} must be positive")
    if cell is not None and not (isinstance(cell, (int, float, np.integer, np.floating)) and not isinstance(cell, bool)
                                 and 0.0 < float(cell) < float("inf")):
        raise ValueError(f"pscv.{what}: cell must be a positive, finite number, got {cell!r}")
    query, xyz = _mesh_points(what, query=query, xyz=xyz)
    _mesh_on_gpu(f"pscv.{what}", query=query, xyz=xyz, faces=faces)
    m, dev = int(query.shape[0]), query.device
    out = torch.full((m,), float("inf"), dtype=torch.float64, device=dev)
    face_out = torch.full((m,), -1, dtype=torch.int32, device=dev) if return_faces else None
    if m and F and V:
        if np.isinf(maxdist):
            # no distance between the queries and the mesh reaches their joint bounding-box diagonal: a finite bound, same results
            lo, hi = _extent(query, xyz)
            maxdist = float(np.linalg.norm(hi - lo)) * 2.0 + 1.0
        origin, fine_cell, coarse_cell = _mesh_cells(xyz, faces, V, maxdist, cell)
        fine = _mesh_grid(xyz, faces, F, V, origin, fine_cell, f"pscv.{what}")
        coarse = _mesh_grid(xyz, faces, F, V, origin, coarse_cell, f"pscv.{what}")
        coarse_rings = int(np.ceil(maxdist / coarse_cell)) + 1
        rc = _launch("mesh_point_dist", lambda: L.lib().pscv_mesh_point_dist(
            _p(query), m, _p(xyz), _p(faces), F, V, _p(fine.buf), fine.pairs, _p(coarse.buf), coarse.pairs, origin[0], origin[1], origin[2],
            fine_cell, coarse_cell, 2, coarse_rings, maxdist, _p(out), _p(face_out), _stream()))
        L.check(rc, "pscv_mesh_point_dist")
    return (out, face_out) if return_faces else out


# --------------------------------------------------------------------------------------------
# fused warp + cost
# --------------------------------------------------------------------------------------------
def warp_cost(ref: Optional[torch.Tensor], srcs: Sequence[torch.Tensor], cams: torch.Tensor, depth: torch.Tensor, *,
              geom: int = L.GEOM_PROJ, cost: int = L.COST_VARIANCE, temp: float = 0.0,
              ref_hw: Optional[Sequence[int]] = None, out_dtype: torch.dtype = torch.bfloat16,
              out: Optional[torch.Tensor] = None, ref_y0: int = 0) -> torch.Tensor:
    """ref [B,h,w,C] (None for WARP_ONLY), srcs n x [B,hs,ws,C], cams [n,B,18] fp32,
    depth [B,D] or [B,D,h,w] fp32  ->  cost volume [B,D,h,w,C]
    (GROUPCORR: [n,B,D,h,w,C/4]; WARP_ONLY: [n,B,D,h,w,C]).  ``ref_y0`` > 0: ``ref`` / per-pixel ``depth`` / the result are rows
    [ref_y0, ref_y0 + h) of a larger reference grid whose cameras ``cams`` are (pscv_warp_cost_rows: bit-identical to those rows of
    the whole-image launch)."""
    srcs = list(srcs)
    _dev(ref, cams, depth, *srcs)
    B, hs, ws, Cc = srcs[0].shape
    for s in srcs:
        if s.shape != srcs[0].shape or s.dtype != srcs[0].dtype:
            raise ValueError("pscv.warp_cost: all source feature maps must share shape and dtype")
    if ref is not None:
        h, w = ref.shape[1:3]
        if ref.dtype != srcs[0].dtype or ref.shape[0] != B or ref.shape[3] != Cc:
            raise ValueError("pscv.warp_cost: ref / src feature mismatch")
    else:
        h, w = (hs, ws) if ref_hw is None else (int(ref_hw[0]), int(ref_hw[1]))
    n = len(srcs)
    if cams.shape != (n, B, L.CAM_FLOATS) or cams.dtype != torch.float32:
        raise ValueError(f"pscv.warp_cost: cams must be fp32 [{n},{B},{L.CAM_FLOATS}], got {tuple(cams.shape)}")
    if depth.dtype != torch.float32:
        raise ValueError("pscv.warp_cost: depth planes must be fp32")
    D = depth.shape[1]
    per_pixel = depth.dim() == 4
    if per_pixel and tuple(depth.shape) != (B, D, h, w):
        raise ValueError("pscv.warp_cost: per-pixel depth must be [B,D,h,w]")
    if not per_pixel and depth.dim() != 2:
        raise ValueError("pscv.warp_cost: depth must be [B,D] or [B,D,h,w]")
    bstride = depth.stride(0)
    if cost == L.COST_GROUPCORR:
        shape = (n, B, D, h, w, Cc // 4)
    elif cost == L.COST_WARP_ONLY:
        shape = (n, B, D, h, w, Cc)
    elif cost == L.COST_VARIANCE_PARTIAL:
        shape, out_dtype = (2, B, D, h, w, Cc), torch.float32     # (sum f, sum f^2) over the given views
    else:
        shape = (B, D, h, w, Cc)
    if out is None:
        out = torch.empty(shape, dtype=out_dtype, device=srcs[0].device)
    elif tuple(out.shape) != shape or not out.is_contiguous():
        raise ValueError("pscv.warp_cost: bad `out` tensor")
    ptrs = (C.c_void_p * n)(*[s.data_ptr() for s in srcs])
    rc = _launch(f"warp_cost[{cost}]", lambda: L.lib().pscv_warp_cost_rows(
        _p(ref), ptrs, n, _p(cams), _p(depth), bstride, int(per_pixel), geom, cost, float(temp), _p(out), B, Cc, h, w,
        hs, ws, D, _dt(srcs[0]), _dt(out), int(ref_y0), _stream()),
        # feature maps once + the volume once; per (voxel, view, channel) 4 blend FMAs + the cost statistic (2 FMAs)
        cost=lambda: (float((n + (ref is not None)) * B * hs * ws * Cc * srcs[0].element_size() + out.numel() * out.element_size()),
                      2.0 * 6 * n * B * D * h * w * Cc))
    L.check(rc, "pscv_warp_cost")
    return out


def variance_finish(sums: torch.Tensor, n_views: int, *, cost: int = L.COST_VARIANCE, dtype: torch.dtype = torch.float16) -> torch.Tensor:
    """(all-reduced) partial sums fp32 [2,B,D,h,w,C] of ``warp_cost(cost=COST_VARIANCE_PARTIAL)`` -> variance volume
    [B,D,h,w,C] in ``dtype`` (pscv_variance_finish)."""
    _dev(sums)
    if sums.dtype != torch.float32 or sums.dim() != 6 or sums.shape[0] != 2 or not sums.is_contiguous():
        raise ValueError("pscv.variance_finish: fp32 [2,B,D,h,w,C] partial sums expected")
    out = torch.empty(tuple(sums.shape[1:]), dtype=dtype, device=sums.device)
    rc = _launch("variance_finish", lambda: L.lib().pscv_variance_finish(_p(sums), out.numel(), int(n_views), cost, _TORCH2PSCV[dtype],
                                                                        _p(out), _stream()))
    L.check(rc, "pscv_variance_finish")
    return out


# --------------------------------------------------------------------------------------------
# conv3d
# --------------------------------------------------------------------------------------------
def pack_conv3d_weights(weight: torch.Tensor, kind: int, transposed: bool,
                        dtype: torch.dtype = torch.bfloat16) -> np.ndarray:
    """Host-side repack of a Conv3d [Co,Ci,3,3,3] / ConvTranspose3d [Ci,Co,3,3,3] weight into the MFMA
    fragment order of the conv kernel (uint16 bit patterns of ``dtype`` = bf16 or fp16)."""
    w = np.ascontiguousarray(weight.detach().to("cpu", torch.float32).numpy())
    if w.ndim != 5 or w.shape[2:] != (3, 3, 3):
        raise ValueError(f"pscv: conv3d weights must be [*,*,3,3,3], got {w.shape}")
    c_in, c_out = (w.shape[0], w.shape[1]) if transposed else (w.shape[1], w.shape[0])
    lib = L.lib()
    code = _TORCH2PSCV.get(dtype, -1)
    n = lib.pscv_pack_conv3d_weights(None, c_in, c_out, kind, int(transposed), code, None)
    if n < 0:
        L.check(int(n), "pscv_pack_conv3d_weights")
    packed = np.empty(n, dtype=np.uint16)
    n2 = lib.pscv_pack_conv3d_weights(w.ctypes.data_as(C.c_void_p), c_in, c_out, kind, int(transposed), code,
                                      packed.ctypes.data_as(C.c_void_p))
    if n2 != n:
        L.check(-1 if n2 >= 0 else int(n2), "pscv_pack_conv3d_weights")
    return packed


def pack_conv3d_weights_device(weight: torch.Tensor, kind: int, transposed: bool, dtype: torch.dtype) -> torch.Tensor:
    """Same repack as ``pack_conv3d_weights`` in one launch on the GPU (pscv_pack_conv3d_weights_device): weights that
    change every optimizer step never travel to the host.  Returns the packed int16 tensor on the weight's device."""
    w = weight.detach().to(torch.float32).contiguous()
    _dev(w)
    if w.dim() != 5 or tuple(w.shape[2:]) != (3, 3, 3):
        raise ValueError(f"pscv: conv3d weights must be [*,*,3,3,3], got {tuple(w.shape)}")
    c_in, c_out = (w.shape[0], w.shape[1]) if transposed else (w.shape[1], w.shape[0])
    code = _TORCH2PSCV.get(dtype, -1)
    n = L.lib().pscv_pack_conv3d_weights(None, c_in, c_out, kind, int(transposed), code, None)
    if n < 0:
        L.check(int(n), "pscv_pack_conv3d_weights")
    packed = torch.empty((n,), dtype=torch.int16, device=w.device)
    rc = _launch("pack_conv3d_weights", lambda: L.lib().pscv_pack_conv3d_weights_device(_p(w), c_in, c_out, kind, int(transposed), code,
                                                                                       _p(packed), _stream()))
    L.check(rc, "pscv_pack_conv3d_weights_device")
    return packed


@dataclass
class Conv3dLayer:
    """One 3x3x3 layer ready for the engine: packed 16-bit weights + fp32 epilogue vectors, on device."""
    packed: torch.Tensor            # int16 bit patterns of the MFMA A fragments
    dtype: torch.dtype              # bf16 or fp16: format of the weights AND of the activations it reads
    c_in: int
    c_out: int
    kind: int
    epi: int
    scale: Optional[torch.Tensor] = None
    bias: Optional[torch.Tensor] = None
    floor: Optional[torch.Tensor] = None

    @staticmethod
    def build(weight: torch.Tensor, *, kind: int, transposed: bool = False, device=None,
              bn: Optional[Sequence[torch.Tensor]] = None, bn_eps: float = 1e-5,
              conv_bias: Optional[torch.Tensor] = None, relu: bool = False, relu_post: bool = False,
              floor: Optional[torch.Tensor] = None, dtype: torch.dtype = torch.bfloat16) -> "Conv3dLayer":
        """``bn`` = (gamma, beta, running_mean, running_var) folds an eval-mode BatchNorm3d into the
        epilogue: scale = gamma / sqrt(var + eps), bias = beta - mean * scale (+ scale * conv_bias)."""
        device = device if device is not None else weight.device
        c_in, c_out = (weight.shape[0], weight.shape[1]) if transposed else (weight.shape[1], weight.shape[0])
        if kind == L.CONV_S1 and ((c_in in (8, 16, 32) and c_out == 8) or (SWEEP16 and (c_in, c_out) == (16, 16))) and USE_SWEEP_KERNEL:
            kind = L.CONV_S1P8     # same result, depth-sweep kernels with plane-pair packed MFMA rows (stride-1 deconvs too)
        # (16 -> 16 has a sweep variant too (kind S1P8 through the C ABI; ``SWEEP16 = True`` selects it), but since the brick kernel's staging / decode rewrite
        #  the brick kernel is faster at every measured size: 295 vs 337 us at 8x1024x1280, 16.6 vs 18.7 us at 96x64x80)
        if kind == L.CONV_T2 and transposed and c_in == 16 and c_out == 8 and USE_SWEEP_KERNEL:
            kind = L.CONV_T2P8     # same result, parity-pair packed MFMA rows + contiguous 32-byte stores
        if kind == L.CONV_S1 and not transposed and c_in in (8, 16) and c_out == 1 and USE_SWEEP_KERNEL:
            kind = L.CONV_S1C1     # same result, depth-in-rows MFMA kernel for the 1-channel heads
        # A training step applies the same Parameter many times (Vis-MVSNet: one pair U-Net per source view and stage, forward and
        # adjoint): raw-weight layers of live Parameters are memoised per parameter VERSION (the optimiser's in-place update bumps
        # it), guarded by a weak reference so that a recycled id() can never alias another tensor.
        ckey = None
        if PACK_CACHE and isinstance(weight, torch.nn.Parameter) and weight.is_cuda and bn is None and conv_bias is None and floor is None:
            ckey = (_weights_epoch, id(weight), kind, bool(transposed), dtype, str(device), bool(relu), bool(relu_post))
            ent = _layer_cache.get(ckey)
            if ent is not None and ent[0]() is weight and ent[1] == weight._version:
                return ent[2]
        if weight.is_cuda and torch.device(device).type == "cuda":
            packed = pack_conv3d_weights_device(weight, kind, transposed, dtype)
        else:
            packed = torch.from_numpy(pack_conv3d_weights(weight, kind, transposed, dtype).view(np.int16)).to(device)
        scale = bias = None
        if bn is not None:
            gamma, beta, mean, var = [t.detach().to(device, torch.float32) for t in bn]
            scale = gamma / torch.sqrt(var + bn_eps)
            bias = beta - mean * scale
            if conv_bias is not None:
                bias = bias + scale * conv_bias.detach().to(device, torch.float32)
            scale, bias = scale.contiguous(), bias.contiguous()
        elif conv_bias is not None:
            bias = conv_bias.detach().to(device, torch.float32).contiguous()
        epi = (L.EPI_RELU_PRE if relu else 0) | (L.EPI_RELU_POST if relu_post else 0)
        if floor is not None:
            floor = floor.detach().to(device, torch.float32).contiguous()
        layer = Conv3dLayer(packed, dtype, int(c_in), int(c_out), kind, epi, scale, bias, floor)
        if ckey is not None:
            if len(_layer_cache) > 4096:
                _layer_cache.clear()
            _layer_cache[ckey] = (weakref.ref(weight), weight._version, layer)
        return layer


USE_SWEEP_KERNEL = True   # tests flip this to compare the two stride-1 kernels
SWEEP16 = False           # 16 -> 16 layers on the depth-sweep kernel (tests / measurements; the brick kernel is the faster one)
_weights_epoch = 0


def weights_epoch() -> int:
    """Generation counter folded into every packed-weight / folded-BatchNorm cache key of the package."""
    return _weights_epoch


def invalidate_weight_caches() -> None:
    """Drop every packed-weight, folded-BatchNorm and soft-min temperature cache of the process.

    The caches are keyed on (storage address, ``tensor._version``): in-place tensor ops, optimiser steps and
    ``load_state_dict`` bump the version and are picked up automatically.  Writes THROUGH ``.data`` (``p.data.copy_(ema)``,
    ``p.data.clamp_()``, old-style optimisers) do not bump it -- call this function (also exported as
    ``wild_deep_mvs_amd.invalidate()``) after such a write, or the engine keeps running the previously packed weights."""
    global _weights_epoch
    _weights_epoch += 1
    _layer_cache.clear()

PACK_CACHE = True         # memoise raw-weight layers of live Parameters per parameter version (Conv3dLayer.build)
_layer_cache: dict = {}


def conv_out_shape(kind: int, D: int, H: int, W: int):
    if kind in (L.CONV_S1, L.CONV_S1P8, L.CONV_S1C1):
        return D, H, W
    if kind == L.CONV_S2:
        return (D + 1) // 2, (H + 1) // 2, (W + 1) // 2
    return 2 * D, 2 * H, 2 * W   # CONV_T2, CONV_T2P8


def _conv_cost(vox_in: int, vox_out: int, c_in: int, c_out: int, taps: int, transposed_s2: bool, out_bytes: int, with_skip: bool):
    """(algorithmic HBM bytes, flops) of one convolution launch: input and output once (+ the skip tensor), 2 x taps x c_in x c_out
    per output voxel (a stride-2 transposed layer touches every input voxel with every tap instead)."""
    b = vox_in * c_in * 2 + vox_out * c_out * out_bytes + (vox_out * c_out * 2 if with_skip else 0)
    f = 2.0 * taps * c_in * c_out * (vox_in if transposed_s2 else vox_out)
    return float(b), f


def conv3d(x: torch.Tensor, layer: Conv3dLayer, *, skip: Optional[torch.Tensor] = None, in_coff: int = 0,
           skip_coff: int = 0, out: Optional[torch.Tensor] = None, out_coff: int = 0,
           out_dtype: Optional[torch.dtype] = None, x2: Optional[torch.Tensor] = None, x2_coff: int = 0) -> torch.Tensor:
    """x [B,D,H,W,Cs] in the layer's 16-bit format (reads channels [in_coff, in_coff+c_in)) ->
    [B,Do,Ho,Wo,c_out] in the same format or fp32 (or writes the channel slice [out_coff, out_coff+c_out)
    of ``out``).  With ``x2`` (16-channel depth-sweep layers) the input is the channel concatenation of
    x[..., in_coff:in_coff+8] and x2[..., x2_coff:x2_coff+8], gathered while staging (pscv_conv3d_cat2)."""
    _dev(x, skip, out, layer.packed)
    if x.dtype != layer.dtype or x.dim() != 5:
        raise TypeError(f"pscv.conv3d: input must be a {layer.dtype} [B,D,H,W,C] volume, got {x.dtype} {tuple(x.shape)}")
    out_dtype = layer.dtype if out_dtype is None else out_dtype
    B, D, H, W, cs = x.shape
    Do, Ho, Wo = conv_out_shape(layer.kind, D, H, W)
    if out is None:
        out = torch.empty((B, Do, Ho, Wo, layer.c_out), dtype=out_dtype, device=x.device)
    if tuple(out.shape[:4]) != (B, Do, Ho, Wo):
        raise ValueError(f"pscv.conv3d: out has shape {tuple(out.shape)}, expected [B,{Do},{Ho},{Wo},*]")
    if skip is not None and (skip.dtype != layer.dtype or tuple(skip.shape[:4]) != (B, Do, Ho, Wo)):
        raise ValueError("pscv.conv3d: skip must have the layer's dtype and the output's spatial shape")
    if x2 is not None:
        # the 16 input channels are cat([x[..., in_coff:in_coff+8], x2[..., x2_coff:x2_coff+8]]) -- never materialised
        _dev(x2)
        if layer.kind != L.CONV_S1P8 or layer.c_in != 16 or x2.dtype != layer.dtype or tuple(x2.shape[:4]) != (B, D, H, W):
            raise ValueError("pscv.conv3d: a second input needs a depth-sweep (S1P8) layer with c_in = 16 and a volume of x's "
                             f"spatial shape in the layer's dtype (layer kind {layer.kind}, c_in {layer.c_in}, x2 {tuple(x2.shape)})")
        rc = _launch(f"conv3d[8+8->{layer.c_out},k{layer.kind}]", lambda: L.lib().pscv_conv3d_cat2(
            _p(x), cs, in_coff, _p(x2), x2.shape[4], x2_coff, _dt(x), _p(layer.packed), _p(layer.scale), _p(layer.bias),
            _p(layer.floor), _p(skip), 0 if skip is None else skip.shape[4], skip_coff, _p(out), out.shape[4], out_coff, _dt(out),
            B, D, H, W, layer.c_out, layer.epi, _stream()),
            cost=lambda: _conv_cost(B * D * H * W, B * Do * Ho * Wo, 16, layer.c_out, 27, False, out.element_size(), skip is not None))
        L.check(rc, "pscv_conv3d_cat2")
        return out
    rc = _launch(f"conv3d[{layer.c_in}->{layer.c_out},k{layer.kind}]", lambda: L.lib().pscv_conv3d(
        _p(x), _dt(x), cs, in_coff, _p(layer.packed), _p(layer.scale), _p(layer.bias), _p(layer.floor), _p(skip),
        0 if skip is None else skip.shape[4], skip_coff, _p(out), out.shape[4], out_coff, _dt(out), B, D, H, W,
        layer.c_in, layer.c_out, layer.kind, layer.epi, _stream()),
        cost=lambda: _conv_cost(B * D * H * W, B * Do * Ho * Wo, layer.c_in, layer.c_out, 27, layer.kind in (L.CONV_T2, getattr(L, "CONV_T2P8", -1)),
                                out.element_size(), skip is not None))
    L.check(rc, "pscv_conv3d")
    return out


def conv3d_block8(x: torch.Tensor, layer1: Conv3dLayer, layer2: Conv3dLayer, *, residual: bool = True, in_coff: int = 0,
                  out: Optional[torch.Tensor] = None, out_coff: int = 0) -> Optional[torch.Tensor]:
    """Two stacked 8 -> 8 depth-sweep layers (+ the block input as residual) in one launch (pscv_conv3d_block8): the values of
    ``conv3d(conv3d(x, layer1), layer2, skip=x)`` without the intermediate volume.  Returns None when the layers are not both
    8 -> 8 depth-sweep (S1P8) layers in x's dtype (run the two launches then)."""
    _dev(x, out, layer1.packed, layer2.packed)
    if not (layer1.kind == layer2.kind == L.CONV_S1P8 and layer1.c_in == layer1.c_out == layer2.c_in == layer2.c_out == 8
            and layer1.dtype == layer2.dtype == x.dtype and x.dim() == 5):
        return None
    B, D, H, W, cs = x.shape
    if out is None:
        out = torch.empty((B, D, H, W, 8), dtype=x.dtype, device=x.device)
    if tuple(out.shape[:4]) != (B, D, H, W) or out.dtype != x.dtype:
        raise ValueError(f"pscv.conv3d_block8: out has shape {tuple(out.shape)} / {out.dtype}, expected [B,{D},{H},{W},*] {x.dtype}")
    vox = B * D * H * W
    rc = _launch("conv3d_block8", lambda: L.lib().pscv_conv3d_block8(
        _p(x), _dt(x), cs, in_coff, _p(layer1.packed), _p(layer1.scale), _p(layer1.bias), _p(layer1.floor), layer1.epi,
        _p(layer2.packed), _p(layer2.scale), _p(layer2.bias), _p(layer2.floor), layer2.epi, int(residual),
        _p(out), out.shape[4], out_coff, B, D, H, W, _stream()),
        cost=lambda: (float(vox * 32), 2.0 * 2 * 27 * 8 * 8 * vox))
    L.check(rc, "pscv_conv3d_block8")
    return out


# --------------------------------------------------------------------------------------------
# Vis-MVSNet UncertNet (eval mode), one launch
# --------------------------------------------------------------------------------------------
def pack_uncert_params(w1, bn1, w2, bn2, head, eps1: float = 1e-5, eps2: float = 1e-5) -> torch.Tensor:
    """The 752-float parameter block of ``pscv_uncert_net`` (include/pscv.h) from the module's tensors: conv weights
    [8,1,3,3], [8,8,3,3], [1,8,3,3]; ``bn*`` = (gamma, beta, running_mean, running_var), folded in fp32."""
    f = lambda t: t.detach().to(torch.float32)

    def fold(bn, eps):
        g, b, m, v = [f(t) for t in bn]
        s = g / torch.sqrt(v + eps)
        return s, b - m * s
    s1, b1 = fold(bn1, eps1)
    s2, b2 = fold(bn2, eps2)
    return torch.cat([f(w1).reshape(8, 9).t().reshape(-1), s1, b1,                     # [tap][co]
                      f(w2).reshape(8, 8, 9).permute(1, 2, 0).reshape(-1), s2, b2,       # [ci][tap][co]
                      f(head).reshape(8, 9).reshape(-1)]).contiguous()                   # [ci][tap]


def uncert_net(entropy: torch.Tensor, params: torch.Tensor) -> torch.Tensor:
    """entropy [N,H,W] fp32 -> log-uncertainty [N,H,W] fp32 (reference model_cas.py:77-98, eval mode)."""
    _dev(entropy, params)
    if entropy.dtype != torch.float32 or entropy.dim() != 3 or not entropy.is_contiguous():
        raise ValueError("pscv.uncert_net: entropy must be a contiguous fp32 [N,H,W] map")
    if params.dtype != torch.float32 or params.numel() != 752 or not params.is_contiguous():
        raise ValueError("pscv.uncert_net: params must be the 752-float block of pack_uncert_params")
    N, H, W = entropy.shape
    out = torch.empty_like(entropy)
    rc = _launch("uncert_net", lambda: L.lib().pscv_uncert_net(_p(entropy), _p(params), _p(out), N, H, W, _stream()))
    L.check(rc, "pscv_uncert_net")
    return out


# --------------------------------------------------------------------------------------------
# softargmin
# --------------------------------------------------------------------------------------------
def softargmin(logits: torch.Tensor, depth: Optional[torch.Tensor] = None, *, want_index: bool = False,
               want_conf: bool = False, conf_mode: int = 0, window: float = 2.0, want_entropy: bool = False,
               want_prob: bool = False, want_partials: bool = False, index_offset: int = 0, into: Optional[dict] = None) -> dict:
    """logits [B,D,h,w] (fp32, bf16 or fp16; 16-bit logits are read as stored and every sum is fp32); depth [B,D] or
    [B,D,h,w] fp32.  Returns a dict with the requested
    maps, each [B,h,w] fp32 (``prob`` [B,D,h,w], ``partials`` [B,4,h,w]).  ``into`` = {name: tensor}: write those maps into
    the caller's contiguous fp32 tensors (e.g. batch slices of one buffer for all source views) instead of new ones.
    torch.softmax semantics: a -inf logit weighs zero; a pixel whose logits are all -inf, or hold NaN or +inf, is NaN in every map."""
    _dev(logits, depth)
    if logits.dim() != 4:
        raise ValueError("pscv.softargmin: logits must be [B,D,h,w]")
    B, D, h, w = logits.shape
    per_pixel = depth is not None and depth.dim() == 4
    if depth is not None:
        if depth.dtype != torch.float32 or depth.shape[:2] != (B, D):
            raise ValueError("pscv.softargmin: depth must be fp32 [B,D] or [B,D,h,w]")
    mk = lambda *s: torch.empty(s, dtype=torch.float32, device=logits.device)
    o = {
        "depth": mk(B, h, w) if depth is not None else None,
        "index": mk(B, h, w) if want_index else None,
        "conf": mk(B, h, w) if want_conf else None,
        "entropy": mk(B, h, w) if want_entropy else None,
        "prob": mk(B, D, h, w) if want_prob else None,
        "partials": mk(B, 4, h, w) if want_partials else None,
    }
    for k, tgt in (into or {}).items():
        if o.get(k) is None or tgt.dtype != torch.float32 or tgt.shape != o[k].shape or not tgt.is_contiguous() or tgt.device != logits.device:
            raise ValueError(f"pscv.softargmin: into[{k!r}] must be a requested map's contiguous fp32 tensor of shape {tuple(o[k].shape) if o.get(k) is not None else None}")
        o[k] = tgt
    rc = _launch("softargmin", lambda: L.lib().pscv_softargmin(
        _p(logits), _dt(logits), _p(depth), 0 if depth is None else depth.stride(0), int(per_pixel), _p(o["depth"]),
        _p(o["index"]), _p(o["conf"]), _p(o["entropy"]), _p(o["prob"]), _p(o["partials"]), conf_mode, float(window),
        index_offset, B, D, h, w, _stream()))
    L.check(rc, "pscv_softargmin")
    return {k: v for k, v in o.items() if v is not None}


_tail_ws: dict = {}       # (device, stream) -> fp32 scratch: launches on different streams must not share partial-sum buffers


def _tail_workspace(device, n: int) -> torch.Tensor:
    key = (device, torch.cuda.current_stream(device).cuda_stream)
    ws = _tail_ws.get(key)
    if ws is None or ws.numel() < n:
        ws = torch.empty(n, dtype=torch.float32, device=device)
        _tail_ws[key] = ws
    return ws


def prob_softargmin(x: torch.Tensor, layer: "Conv3dLayer", depth: torch.Tensor, *, in_coff: int = 0, want_conf: bool = True):
    """Fused tail of the MVSNet regulariser (pscv_prob_softargmin): x [B,D,h,w,Cs] 16-bit -> the 1-channel head ``layer`` (kind
    S1C1, c_in 8) -> fp32 logits [B,D,h,w] + depth [B,h,w] (+ 4-plane confidence), with per-batch depth planes ``depth`` [B,D].
    Returns None when the layer / size does not run the depth-sweep head (call ``conv3d`` + ``softargmin`` then)."""
    _dev(x, depth, layer.packed)
    if layer.kind != L.CONV_S1C1 or layer.c_in != 8 or x.dtype != layer.dtype or x.dim() != 5 or depth.dim() != 2 \
            or depth.dtype != torch.float32:
        return None
    B, D, H, W, cs = x.shape
    if tuple(depth.shape) != (B, D) or D < 18:
        return None
    n = int(L.lib().pscv_prob_softargmin_workspace(B, D, H, W))
    ws = _tail_workspace(x.device, n)
    logits = torch.empty((B, D, H, W), dtype=torch.float32, device=x.device)
    o_depth = torch.empty((B, H, W), dtype=torch.float32, device=x.device)
    o_conf = torch.empty((B, H, W), dtype=torch.float32, device=x.device) if want_conf else None
    rc = _launch("prob_softargmin", lambda: L.lib().pscv_prob_softargmin(
        _p(x), _dt(x), cs, in_coff, _p(layer.packed), _p(layer.scale), _p(layer.bias), _p(layer.floor), layer.c_in, layer.epi,
        _p(depth), depth.stride(0), _p(logits), _p(ws), ws.numel(), _p(o_depth), _p(o_conf), B, D, H, W, _stream()))
    if rc == -3:
        return None
    L.check(rc, "pscv_prob_softargmin")
    out = {"logits": logits, "depth": o_depth}
    if want_conf:
        out["conf"] = o_conf
    return out


def tail_sweep(x: torch.Tensor, up: "Conv3dLayer", head: "Conv3dLayer", *, skip: Optional[torch.Tensor] = None, in_coff: int = 0,
               skip_coff: int = 0, regress: Optional[torch.Tensor] = None, want_conf: bool = True):
    """Fused tail of the MVSNet regulariser (pscv_tail_sweep): x [B,Di,Hi,Wi,Cs] 16-bit -> transposed layer ``up`` (kind T2P8,
    16 -> 8, + ``skip`` [B,2Di,2Hi,2Wi,*]) -> 1-channel head ``head`` (kind S1C1) -> fp32 logits [B,2Di,2Hi,2Wi]; the 8-channel
    full-resolution volume is never stored.  Same bits as ``conv3d(conv3d(x, up, skip=skip), head, out_dtype=float32)``.
    With ``regress`` = per-batch depth planes [B,2Di] the sweep also keeps softmax statistics and a merge launch regresses depth
    (and the 4-plane confidence): returns {"logits", "depth", "conf"} -- no separate softargmin pass.  Returns None when the
    layers / shape are not covered (run the two layers then)."""
    _dev(x, skip, up.packed, head.packed, regress)
    if (up.kind != L.CONV_T2P8 or head.kind != L.CONV_S1C1 or up.c_in != 16 or up.c_out != 8 or head.c_in != 8 or x.dim() != 5
            or x.dtype != up.dtype or head.dtype != up.dtype or (skip is not None and skip.dtype != x.dtype)):
        return None
    B, Di, Hi, Wi, cs = x.shape
    if skip is not None and tuple(skip.shape[:4]) != (B, 2 * Di, 2 * Hi, 2 * Wi):
        raise ValueError(f"pscv.tail_sweep: skip has shape {tuple(skip.shape)}, expected [B,{2 * Di},{2 * Hi},{2 * Wi},*]")
    if regress is not None and (regress.dtype != torch.float32 or tuple(regress.shape) != (B, 2 * Di)):
        raise ValueError(f"pscv.tail_sweep: regress must be fp32 depth planes [B,{2 * Di}]")
    logits = torch.empty((B, 2 * Di, 2 * Hi, 2 * Wi), dtype=torch.float32, device=x.device)
    ws = o_depth = o_conf = None
    if regress is not None:
        ws = _tail_workspace(x.device, int(L.lib().pscv_tail_sweep_workspace(B, Di, Hi, Wi)))
        o_depth = torch.empty((B, 2 * Hi, 2 * Wi), dtype=torch.float32, device=x.device)
        o_conf = torch.empty((B, 2 * Hi, 2 * Wi), dtype=torch.float32, device=x.device) if want_conf else None
    vox = B * 8 * Di * Hi * Wi
    rc = _launch("tail_sweep", lambda: L.lib().pscv_tail_sweep(
        _p(x), _dt(x), cs, in_coff, _p(up.packed), _p(up.scale), _p(up.bias), _p(up.floor), up.epi, _p(skip),
        skip.shape[4] if skip is not None else 0, skip_coff, _p(head.packed), _p(head.scale), _p(head.bias), _p(head.floor), head.epi,
        _p(logits), _p(regress), regress.stride(0) if regress is not None else 0, _p(ws), ws.numel() if ws is not None else 0,
        _p(o_depth), _p(o_conf), B, Di, Hi, Wi, _stream()),
        cost=lambda: (vox // 8 * 32 + vox * (16 if skip is not None else 0) + vox * 4, 2.0 * vox * 27 * 8 + 2.0 * (vox // 8) * 27 * 16 * 8))
    if rc == 1:
        return None
    L.check(rc, "pscv_tail_sweep")
    if regress is None:
        return logits
    out = {"logits": logits, "depth": o_depth}
    if want_conf:
        out["conf"] = o_conf
    return out


def head_index_entropy(x: torch.Tensor, layer: "Conv3dLayer", index: torch.Tensor, entropy: torch.Tensor, *, want_scores: bool = False):
    """Fused head of a Vis pair branch (pscv_head_index_entropy): x [B,D,h,w,8] 16-bit -> the 1-channel head ``layer`` (kind S1C1)
    -> expected plane index and entropy written into the caller's fp32 [B,h,w] tensors; the fp32 scores only with
    ``want_scores``.  Returns None when the layer / size does not run the depth-sweep head (call ``conv3d`` + ``softargmin``
    then), else the scores or True."""
    _dev(x, layer.packed, index, entropy)
    if layer.kind != L.CONV_S1C1 or layer.c_in != 8 or x.dtype != layer.dtype or x.dim() != 5:
        return None
    B, D, H, W, cs = x.shape
    for t_ in (index, entropy):
        if t_.dtype != torch.float32 or tuple(t_.shape) != (B, H, W) or not t_.is_contiguous():
            raise ValueError("pscv.head_index_entropy: index / entropy must be contiguous fp32 [B,h,w] tensors")
    n = int(L.lib().pscv_prob_softargmin_workspace(B, D, H, W))
    ws = _tail_workspace(x.device, n)
    scores = torch.empty((B, D, H, W), dtype=torch.float32, device=x.device) if want_scores else None
    rc = _launch("head_index_entropy", lambda: L.lib().pscv_head_index_entropy(
        _p(x), _dt(x), cs, 0, _p(layer.packed), _p(layer.scale), _p(layer.bias), _p(layer.floor), layer.c_in, layer.epi,
        _p(scores), _p(ws), ws.numel(), _p(index), _p(entropy), B, D, H, W, _stream()),
        cost=lambda: (B * D * H * W * (16 + (4 if want_scores else 0)), 2.0 * B * D * H * W * 27 * 8))
    if rc == -3:
        return None
    L.check(rc, "pscv_head_index_entropy")
    return scores if want_scores else True


def softargmin_window(logits: torch.Tensor, stats: torch.Tensor, *, window: float, index_offset: int) -> torch.Tensor:
    """One depth shard's part of the +-window probability under globally merged softmax statistics: logits fp32 [B,D,h,w] (this
    shard's planes), stats fp32 [B,3,h,w] = (max, sum exp, expected index) -> fp32 [B,h,w] (pscv_softargmin_window)."""
    _dev(logits, stats)
    B, D, h, w = logits.shape
    if logits.dtype != torch.float32 or stats.dtype != torch.float32 or tuple(stats.shape) != (B, 3, h, w):
        raise ValueError("pscv.softargmin_window: fp32 logits [B,D,h,w] and stats [B,3,h,w] expected")
    out = torch.empty((B, h, w), dtype=torch.float32, device=logits.device)
    rc = _launch("softargmin_window", lambda: L.lib().pscv_softargmin_window(_p(logits), _p(stats), _p(out), float(window),
                                                                            int(index_offset), B, D, h, w, _stream()))
    L.check(rc, "pscv_softargmin_window")
    return out


# --------------------------------------------------------------------------------------------
# unsupervised photometric loss: depth -> flows -> warped sources, SSIM
# --------------------------------------------------------------------------------------------
def inv_proj4x4(P: torch.Tensor) -> torch.Tensor:
    """Inverse of projection matrices [...,4,4] with last row (0,0,0,1): [[A^-1, -A^-1 b], [0 0 0 1]], closed form in fp64
    (the reference calls torch.inverse in fp32, utils_3D.py:196; no LAPACK call / host sync here)."""
    Pd = P.double()
    Ai = inv3x3(Pd[..., :3, :3])
    out = torch.zeros_like(Pd)
    out[..., :3, :3] = Ai
    out[..., :3, 3:] = -(Ai @ Pd[..., :3, 3:])
    out[..., 3, 3] = 1.0
    return out.to(P.dtype)


def _photo_args(src_imgs, depth, inv_ref, proj_src):
    _dev(depth, inv_ref, proj_src)
    B, h, w = depth.shape
    S = proj_src.shape[1]
    if depth.dtype != torch.float32 or inv_ref.dtype != torch.float32 or proj_src.dtype != torch.float32 \
            or tuple(inv_ref.shape) != (B, 4, 4) or tuple(proj_src.shape) != (B, S, 4, 4):
        raise ValueError("pscv.photo_warp: fp32 depth [B,h,w], inv_ref [B,4,4], proj_src [B,S,4,4] expected")
    C = 0
    if src_imgs is not None:
        _dev(src_imgs)
        C = src_imgs.shape[2]
        if src_imgs.dtype != torch.float32 or tuple(src_imgs.shape) != (B, S, C, h, w):
            raise ValueError(f"pscv.photo_warp: source images fp32 [B,S,C,h,w] at the depth map's resolution expected, got "
                             f"{tuple(src_imgs.shape)} for depth {tuple(depth.shape)}")
    return B, S, C, h, w


def photo_warp(src_imgs: Optional[torch.Tensor], depth: torch.Tensor, inv_ref: torch.Tensor, proj_src: torch.Tensor, *,
               src_depth: Optional[torch.Tensor] = None, want_mask: bool = True, want_z: bool = False, want_flows: bool = False) -> dict:
    """Depth map -> flows -> warped sources (pscv_photo_warp; trainer.py:209-236).  Returns a dict with ``warped`` [B,S,C,h,w]
    (if images are given), ``mask`` [B,S,h,w] fp32, ``z`` [B,S,h,w], ``flows`` [B,S,h,w,2], ``warped_depth`` [B,S,h,w]."""
    B, S, C, h, w = _photo_args(src_imgs, depth, inv_ref, proj_src)
    depth, inv_ref, proj_src = depth.contiguous(), inv_ref.contiguous(), proj_src.contiguous()
    mk = lambda *sh: torch.empty(sh, dtype=torch.float32, device=depth.device)
    o = {"warped": mk(B, S, C, h, w) if src_imgs is not None else None, "mask": mk(B, S, h, w) if want_mask else None,
         "z": mk(B, S, h, w) if want_z else None, "flows": mk(B, S, h, w, 2) if want_flows else None,
         "warped_depth": mk(B, S, h, w) if src_depth is not None else None}
    if src_imgs is not None:
        src_imgs = src_imgs.contiguous()
    if src_depth is not None:
        _dev(src_depth)
        if src_depth.dtype != torch.float32 or tuple(src_depth.shape) != (B, S, h, w):
            raise ValueError("pscv.photo_warp: src_depth fp32 [B,S,h,w] expected")
        src_depth = src_depth.contiguous()
    rc = _launch("photo_warp", lambda: L.lib().pscv_photo_warp(_p(src_imgs), _p(depth), _p(inv_ref), _p(proj_src), _p(src_depth),
                                                              _p(o["warped"]), _p(o["mask"]), _p(o["z"]), _p(o["flows"]),
                                                              _p(o["warped_depth"]), B, S, C, h, w, _stream()))
    L.check(rc, "pscv_photo_warp")
    return o


def photo_warp_bwd(src_imgs: torch.Tensor, depth: torch.Tensor, inv_ref: torch.Tensor, proj_src: torch.Tensor,
                   grad_warped: torch.Tensor) -> torch.Tensor:
    """grad_warped [B,S,C,h,w] -> grad_depth [B,h,w] (pscv_photo_warp_bwd)."""
    B, S, C, h, w = _photo_args(src_imgs, depth, inv_ref, proj_src)
    _dev(grad_warped)
    if grad_warped.dtype != torch.float32 or tuple(grad_warped.shape) != (B, S, C, h, w):
        raise ValueError("pscv.photo_warp_bwd: grad_warped fp32 [B,S,C,h,w] expected")
    gd = torch.empty((B, h, w), dtype=torch.float32, device=depth.device)
    src_imgs, depth, inv_ref, proj_src, grad_warped = (t.contiguous() for t in (src_imgs, depth, inv_ref, proj_src, grad_warped))
    rc = _launch("photo_warp_bwd", lambda: L.lib().pscv_photo_warp_bwd(_p(src_imgs), _p(depth), _p(inv_ref), _p(proj_src),
                                                                      _p(grad_warped), _p(gd), B, S, C, h, w, _stream()))
    L.check(rc, "pscv_photo_warp_bwd")
    return gd


def _ssim_args(img1, img2):
    _dev(img1, img2)
    if img1.dtype != torch.float32 or img2.dtype != torch.float32 or img1.dim() != 4 or img2.dim() != 4 \
            or img1.shape[1:] != img2.shape[1:] or img2.shape[0] % img1.shape[0]:
        raise ValueError(f"pscv.ssim: fp32 img1 [n1,C,h,w] and img2 [n1*rep,C,h,w] expected, got {tuple(img1.shape)} {tuple(img2.shape)}")
    n1, C, h, w = img1.shape
    return n1, img2.shape[0] // n1, C, h, w


def ssim(img1: torch.Tensor, img2: torch.Tensor) -> torch.Tensor:
    """1 - SSIM per channel (pscv_ssim; utils/ssimLoss.py:27-60): img1 [n1,C,h,w], img2 [n1*rep,C,h,w] -> [n1*rep,C,h,w]."""
    n1, rep, C, h, w = _ssim_args(img1, img2)
    img1, img2 = img1.contiguous(), img2.contiguous()
    out = torch.empty_like(img2)
    rc = _launch("ssim", lambda: L.lib().pscv_ssim(_p(img1), _p(img2), _p(out), n1, rep, C, h, w, _stream()))
    L.check(rc, "pscv_ssim")
    return out


def ssim_bwd(img1: torch.Tensor, img2: torch.Tensor, grad_out: torch.Tensor) -> torch.Tensor:
    """Gradient of ``ssim`` to img2 (pscv_ssim_bwd)."""
    n1, rep, C, h, w = _ssim_args(img1, img2)
    _dev(grad_out)
    if grad_out.dtype != torch.float32 or grad_out.shape != img2.shape:
        raise ValueError("pscv.ssim_bwd: grad_out must match img2")
    img1, img2, grad_out = img1.contiguous(), img2.contiguous(), grad_out.contiguous()
    ws = torch.empty((3 * img2.numel(),), dtype=torch.float32, device=img2.device)
    g2 = torch.empty_like(img2)
    rc = _launch("ssim_bwd", lambda: L.lib().pscv_ssim_bwd(_p(img1), _p(img2), _p(grad_out), _p(ws), _p(g2), n1, rep, C, h, w, _stream()))
    L.check(rc, "pscv_ssim_bwd")
    return g2


# --------------------------------------------------------------------------------------------
# CVP refinement hypotheses
# --------------------------------------------------------------------------------------------
def cvp_depth_hypos(depth: torch.Tensor, cams: torch.Tensor, fallback: torch.Tensor, *, want_steps: bool = False):
    """depth fp32 [B,H,W], cams fp64 [B,39] (K_ref^-1, rows 0..2 of E_src E_ref^-1, K_src, (K_ref R_ref)(K_src R_src)^-1),
    fallback fp32 [B] -> hypotheses fp32 [B,8,H,W] = depth + k * median|step| (pscv_cvp_depth_hypos; no host sync)."""
    _dev(depth, cams, fallback)
    if depth.dtype != torch.float32 or depth.dim() != 3 or cams.dtype != torch.float64 or tuple(cams.shape) != (depth.shape[0], 39) \
            or fallback.dtype != torch.float32 or fallback.numel() != depth.shape[0]:
        raise ValueError("pscv.cvp_depth_hypos: depth fp32 [B,H,W], cams fp64 [B,39], fallback fp32 [B] expected")
    B, H, W = depth.shape
    keys = torch.empty((B * H * W + B * 1040,), dtype=torch.int64, device=depth.device)
    steps = torch.empty((B,), dtype=torch.float64, device=depth.device)
    hypos = torch.empty((B, 8, H, W), dtype=torch.float32, device=depth.device)
    rc = _launch("cvp_depth_hypos", lambda: L.lib().pscv_cvp_depth_hypos(_p(depth), _p(cams), _p(fallback), _p(keys), _p(steps),
                                                                        _p(hypos), B, H, W, _stream()))
    L.check(rc, "pscv_cvp_depth_hypos")
    return (hypos, steps) if want_steps else hypos


def homography_warp(image_cl: torch.Tensor, H: torch.Tensor, ref_hw: Sequence[int]) -> torch.Tensor:
    """image fp32 channels-last [m,hs,ws,c]; H fp32 [m,3,3] (one per batch item) or [m,h,w,3,3] (one per reference pixel)
    -> warped fp32 [m,h,w,c] (pscv_homography_warp)."""
    _dev(image_cl, H)
    if image_cl.dtype != torch.float32 or image_cl.dim() != 4 or H.dtype != torch.float32:
        raise TypeError("pscv.homography_warp: fp32 channels-last image [m,hs,ws,c] and fp32 homographies expected")
    m, hs, ws, c = image_cl.shape
    h, w = int(ref_hw[0]), int(ref_hw[1])
    per_pixel = H.dim() == 5
    if tuple(H.shape) not in ((m, 3, 3), (m, h, w, 3, 3)):
        raise ValueError(f"pscv.homography_warp: H must be [{m},3,3] or [{m},{h},{w},3,3], got {tuple(H.shape)}")
    out = torch.empty((m, h, w, c), dtype=torch.float32, device=image_cl.device)
    rc = _launch("homography_warp", lambda: L.lib().pscv_homography_warp(_p(image_cl), _p(H), int(per_pixel), _p(out), m, c, h, w, hs,
                                                                       ws, _stream()))
    L.check(rc, "pscv_homography_warp")
    return out


def homography_warp_bwd(grad_out: torch.Tensor, H: torch.Tensor, src_hw: Sequence[int]) -> torch.Tensor:
    """Adjoint of ``homography_warp`` w.r.t. the image: grad_out fp32 [m,h,w,c], H as in the forward -> grad_image fp32 [m,hs,ws,c]
    (pscv_homography_warp_bwd; reference: autograd of grid_sample's input, models/VisMVSNet/homography.py:101-102)."""
    _dev(grad_out, H)
    if grad_out.dtype != torch.float32 or grad_out.dim() != 4 or H.dtype != torch.float32:
        raise TypeError("pscv.homography_warp_bwd: fp32 channels-last gradient [m,h,w,c] and fp32 homographies expected")
    grad_out = grad_out.contiguous()
    m, h, w, c = grad_out.shape
    hs, ws = int(src_hw[0]), int(src_hw[1])
    per_pixel = H.dim() == 5
    if tuple(H.shape) not in ((m, 3, 3), (m, h, w, 3, 3)):
        raise ValueError(f"pscv.homography_warp_bwd: H must be [{m},3,3] or [{m},{h},{w},3,3], got {tuple(H.shape)}")
    gimg = torch.zeros((m, hs, ws, c), dtype=torch.float32, device=grad_out.device)
    rc = _launch("homography_warp_bwd", lambda: L.lib().pscv_homography_warp_bwd(_p(grad_out), _p(H), int(per_pixel), _p(gimg), m, c, h, w,
                                                                               hs, ws, _stream()))
    L.check(rc, "pscv_homography_warp_bwd")
    return gimg


def cvp_cams(ref_in: torch.Tensor, src_in: torch.Tensor, ref_ex: torch.Tensor, src_ex: torch.Tensor, level_scales: Sequence[float],
             *, want_hypo: bool = True):
    """All camera blocks of a CVP-MVSNet forward in one launch (pscv_cvp_cams): ref_in [B,3,3], src_in [B,N,3,3], ref_ex [B,4,4],
    src_ex [B,N,4,4]; ``level_scales[l]`` = image_height / level_height.  Returns (warp cams fp32 [L,N,B,18] -- ``warp[l]`` is the
    ``cams`` of ``warp_cost`` at level l --, hypothesis cams fp64 [L,B,39] for ``cvp_depth_hypos`` or None)."""
    f32 = lambda t: t.detach().to(torch.float32).contiguous()
    ref_in, src_in, ref_ex, src_ex = f32(ref_in), f32(src_in), f32(ref_ex), f32(src_ex)
    _dev(ref_in, src_in, ref_ex, src_ex)
    B, N = src_in.shape[:2]
    if tuple(ref_in.shape) != (B, 3, 3) or tuple(src_in.shape) != (B, N, 3, 3) or tuple(ref_ex.shape) != (B, 4, 4) \
            or tuple(src_ex.shape) != (B, N, 4, 4):
        raise ValueError("pscv.cvp_cams: ref_in [B,3,3], src_in [B,N,3,3], ref_ex [B,4,4], src_ex [B,N,4,4] expected")
    nl = len(level_scales)
    sc = (C.c_float * nl)(*[float(v) for v in level_scales])
    warp = torch.empty((nl, N, B, L.CAM_FLOATS), dtype=torch.float32, device=ref_in.device)
    hypo = torch.empty((nl, B, 39), dtype=torch.float64, device=ref_in.device) if want_hypo else None
    rc = _launch("cvp_cams", lambda: L.lib().pscv_cvp_cams(_p(ref_in), _p(src_in), _p(ref_ex), _p(src_ex), sc, B, N, nl, _p(warp),
                                                         _p(hypo), _stream()))
    L.check(rc, "pscv_cvp_cams")
    return warp, hypo


# --------------------------------------------------------------------------------------------
# training path: batch-statistics BatchNorm pieces, weight gradients, backward of the sweep
# --------------------------------------------------------------------------------------------
_train_ws = {}


def _workspace(device, nfloats: int) -> torch.Tensor:
    """fp32 scratch for the two-phase reductions, one per (device, stream), grown on demand: reuse is ordered by the stream, and
    launches on different streams (round-3 advisor finding: the batch stream mode) never share a partial-sum buffer."""
    key = (device, torch.cuda.current_stream(device).cuda_stream)
    ws = _train_ws.get(key)
    if ws is None or ws.numel() < nfloats:
        ws = torch.empty(max(int(nfloats), int(L.lib().pscv_train_workspace_floats())), dtype=torch.float32, device=device)
        _train_ws[key] = ws
    return ws


def _vol16(x: torch.Tensor, what: str):
    if x.dtype not in HALF_DTYPES or x.dim() != 5 or x.shape[4] not in (8, 16, 32, 64, 128):
        raise TypeError(f"pscv.{what}: a 16-bit channels-last volume [B,D,h,w,C] with C in 8/16/32/64/128 is expected, got "
                        f"{x.dtype} {tuple(x.shape)}")


def _group_vox(y: torch.Tensor, groups: int, what: str) -> int:
    """Voxels per group of a contiguous volume whose leading (batch) axis holds ``groups`` equal consecutive slices."""
    if groups < 1 or y.shape[0] % groups or not y.is_contiguous():
        raise ValueError(f"pscv.{what}: {groups} groups need a contiguous volume whose batch axis ({y.shape[0]}) they divide")
    return y.numel() // y.shape[4] // groups


def _dev_rows(*ts: Optional[torch.Tensor]):
    """Per-channel constants: device tensors whose channel axis is dense (a [C] vector, or [G,C] rows of a larger tensor)."""
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError("pscv: the plane-sweep engine runs on MI355X only; got a CPU tensor")
        if t.stride(-1) != 1 or (t.dim() == 1 and not t.is_contiguous()):
            raise ValueError("pscv: per-channel constants must be dense along the channel axis")


def _row_stride(a: torch.Tensor, b: torch.Tensor, groups: int, Cc: int, what: str, c: Optional[torch.Tensor] = None) -> int:
    """Per-group constants handed over as [G,C] views of one [G,k,C] tensor: the float stride between groups (the same for all)."""
    ts = [t for t in (a, b, c) if t is not None]
    for t in ts:
        if t.dtype != torch.float32 or t.shape != (groups, Cc) or t.stride(1) != 1 or t.stride(0) != ts[0].stride(0):
            raise ValueError(f"pscv.{what}: per-group constants must be fp32 [groups,C] rows with one common group stride")
    return int(ts[0].stride(0))


def bn_stats(y: torch.Tensor, groups: int = 1) -> torch.Tensor:
    """y [B,D,h,w,C] 16-bit -> fp32 [2,C]: per-channel sum and sum of squares over all voxels (pscv_bn_stats).  ``groups`` > 1:
    the batch axis is ``groups`` consecutive slices with their own statistics (the views of a 2-D extractor batch) -> [groups,2,C]."""
    _dev(y)
    _vol16(y, "bn_stats")
    Cc = y.shape[4]
    nv = _group_vox(y, groups, "bn_stats")
    sums = torch.empty((2, Cc) if groups == 1 else (groups, 2, Cc), dtype=torch.float32, device=y.device)
    ws = _workspace(y.device, 0)
    rc = _launch("bn_stats", lambda: L.lib().pscv_bn_stats_grouped(_p(y), _dt(y), nv, groups, Cc, _p(ws), _p(sums), _stream()))
    L.check(rc, "pscv_bn_stats")
    return sums


def bn_finalize(sums: torch.Tensor, nvox: int, bn) -> torch.Tensor:
    """sums fp32 [2,C] of ``bn_stats`` -> fp32 [4,C] = (scale, bias, mean, invstd) of a BatchNorm module in train(); updates its
    running statistics and ``num_batches_tracked`` like nn.BatchNorm3d (pscv_bn_finalize, one launch).  Grouped sums [G,2,C]
    (``nvox`` per group) -> [G,4,C]; the running statistics are updated once per group, in order, as G forward calls would."""
    _dev(sums)
    groups = 1 if sums.dim() == 2 else sums.shape[0]
    Cc = sums.shape[-1]
    out = torch.empty((4, Cc) if sums.dim() == 2 else (groups, 4, Cc), dtype=torch.float32, device=sums.device)
    track = bn.track_running_stats and bn.running_mean is not None
    if track and bn.momentum is None:
        raise NotImplementedError("pscv BatchNorm training: cumulative moving average (momentum=None) is not used by the reference")
    f32 = lambda t_: None if t_ is None else (t_ if t_.dtype == torch.float32 else t_.detach().float())
    gamma, beta = f32(bn.weight), f32(bn.bias)
    rm, rv = (bn.running_mean, bn.running_var) if track else (None, None)
    if track and (rm.dtype != torch.float32 or rv.dtype != torch.float32):
        raise TypeError("pscv BatchNorm training: fp32 running statistics expected")
    nbt = bn.num_batches_tracked if track else None
    rc = _launch("bn_finalize", lambda: L.lib().pscv_bn_finalize_grouped(_p(sums), int(nvox), groups, Cc, _p(gamma), _p(beta), float(bn.eps),
                                                                        float(bn.momentum if track else 0.0), _p(rm), _p(rv), _p(nbt), _p(out),
                                                                        _stream()))
    L.check(rc, "pscv_bn_finalize")
    return out


def bn_bwd_coeffs(sums: torch.Tensor, mean: torch.Tensor, invstd: torch.Tensor, gamma: Optional[torch.Tensor], nvox: int) -> torch.Tensor:
    """sums fp32 [2,C] of ``bn_bwd_reduce`` -> fp32 [5,C] = (ca, cb, cc, d gamma, d beta) (pscv_bn_bwd_coeffs, one launch).
    Grouped: sums [G,2,C], ``mean`` / ``invstd`` = rows 2 / 3 of ``bn_finalize``'s [G,4,C] (views) -> [G,5,C]."""
    _dev(sums, gamma)
    _dev_rows(mean, invstd)
    groups = 1 if sums.dim() == 2 else sums.shape[0]
    Cc = sums.shape[-1]
    out = torch.empty((5, Cc) if sums.dim() == 2 else (groups, 5, Cc), dtype=torch.float32, device=sums.device)
    g = None if gamma is None else (gamma.detach() if gamma.dtype == torch.float32 else gamma.detach().float())
    sst = 0 if groups == 1 else _row_stride(mean, invstd, groups, Cc, "bn_bwd_coeffs")
    rc = _launch("bn_bwd_coeffs", lambda: L.lib().pscv_bn_bwd_coeffs_grouped(_p(sums), _p(mean), _p(invstd), sst, _p(g), int(nvox), groups, Cc,
                                                                            _p(out), _stream()))
    L.check(rc, "pscv_bn_bwd_coeffs")
    return out


def bn_act(y: torch.Tensor, scale: torch.Tensor, bias: torch.Tensor, *, relu, skip: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[relu](y * scale + bias) + skip on a 16-bit channels-last volume (pscv_bn_act).  ``relu``: False / True (before the
    skip add) / "post" (after it: the Vis BasicBlock)."""
    _dev(y, skip)
    _dev_rows(scale, bias)
    _vol16(y, "bn_act")
    if skip is not None and (skip.shape != y.shape or skip.dtype != y.dtype):
        raise ValueError("pscv.bn_act: skip must match y")
    Cc = y.shape[4]
    groups = 1 if scale.dim() == 1 else scale.shape[0]          # grouped: scale / bias [G,C] (rows of bn_finalize's [G,4,C])
    nv = _group_vox(y, groups, "bn_act") if groups > 1 else y.numel() // Cc
    pst = 0 if groups == 1 else _row_stride(scale, bias, groups, Cc, "bn_act")
    out = torch.empty_like(y)
    rc = _launch("bn_act", lambda: L.lib().pscv_bn_act_grouped(_p(y), _dt(y), nv, groups, Cc, _p(scale), _p(bias), pst,
                                                              2 if relu == "post" else int(bool(relu)), _p(skip), _p(out), _stream()))
    L.check(rc, "pscv_bn_act")
    return out


def bn_bwd_reduce(dact: torch.Tensor, y: torch.Tensor, scale: torch.Tensor, bias: torch.Tensor, *, relu: bool) -> torch.Tensor:
    """fp32 [2,C]: sum dz and sum dz*y with dz = dact * [y*scale+bias > 0] (pscv_bn_bwd_reduce)."""
    _dev(dact, y)
    _dev_rows(scale, bias)
    _vol16(y, "bn_bwd_reduce")
    if dact.shape != y.shape or dact.dtype != y.dtype:
        raise ValueError("pscv.bn_bwd_reduce: dact must match y")
    Cc = y.shape[4]
    groups = 1 if scale.dim() == 1 else scale.shape[0]
    nv = _group_vox(y, groups, "bn_bwd_reduce") if groups > 1 else y.numel() // Cc
    pst = 0 if groups == 1 else _row_stride(scale, bias, groups, Cc, "bn_bwd_reduce")
    if not dact.is_contiguous():
        raise ValueError("pscv.bn_bwd_reduce: dact must be contiguous")
    sums = torch.empty((2, Cc) if scale.dim() == 1 else (groups, 2, Cc), dtype=torch.float32, device=y.device)
    ws = _workspace(y.device, 0)
    rc = _launch("bn_bwd_reduce", lambda: L.lib().pscv_bn_bwd_reduce_grouped(_p(dact), _p(y), _dt(y), nv, groups, Cc, _p(scale), _p(bias), pst,
                                                                            int(relu), _p(ws), _p(sums), _stream()))
    L.check(rc, "pscv_bn_bwd_reduce")
    return sums


def bn_bwd_apply(dact: torch.Tensor, y: torch.Tensor, scale: torch.Tensor, bias: torch.Tensor, ca: torch.Tensor, cb: torch.Tensor,
                 cc: torch.Tensor, *, relu: bool) -> torch.Tensor:
    """dy = ca * dz + cb * y + cc per channel (pscv_bn_bwd_apply)."""
    _dev(dact, y)
    _dev_rows(scale, bias, ca, cb, cc)
    _vol16(y, "bn_bwd_apply")
    Cc = y.shape[4]
    groups = 1 if scale.dim() == 1 else scale.shape[0]
    nv = _group_vox(y, groups, "bn_bwd_apply") if groups > 1 else y.numel() // Cc
    pst = 0 if groups == 1 else _row_stride(scale, bias, groups, Cc, "bn_bwd_apply")
    cst = 0 if groups == 1 else _row_stride(ca, cb, groups, Cc, "bn_bwd_apply", cc)
    dy = torch.empty_like(y)
    rc = _launch("bn_bwd_apply", lambda: L.lib().pscv_bn_bwd_apply_grouped(_p(dact), _p(y), _dt(y), nv, groups, Cc, _p(scale), _p(bias), pst,
                                                                          int(relu), _p(ca), _p(cb), _p(cc), cst, _p(dy), _stream()))
    L.check(rc, "pscv_bn_bwd_apply")
    return dy


def softargmin_bwd(logits: torch.Tensor, depth: Optional[torch.Tensor], grad_depth: Optional[torch.Tensor], dtype: torch.dtype, *,
                   grad_index: Optional[torch.Tensor] = None, grad_entropy: Optional[torch.Tensor] = None) -> torch.Tensor:
    """logits fp32 [B,D,h,w]; upstream gradients fp32 [B,h,w] of depth (needs the planes [B,D] / [B,D,h,w]), expected index
    and entropy (each optional) -> [B,D,h,w,8] in ``dtype`` with d loss / d logit in channel 0 and zeros elsewhere
    (pscv_softargmin_bwd)."""
    _dev(logits, depth, grad_depth, grad_index, grad_entropy)
    if logits.dtype != torch.float32 or logits.dim() != 4:
        raise TypeError("pscv.softargmin_bwd: fp32 logits [B,D,h,w] expected")
    B, D, h, w = logits.shape
    for g in (grad_depth, grad_index, grad_entropy):
        if g is not None and (g.dtype != torch.float32 or tuple(g.shape) != (B, h, w)):
            raise ValueError("pscv.softargmin_bwd: upstream gradients must be fp32 [B,h,w]")
    if grad_depth is not None and (depth is None or depth.dtype != torch.float32 or depth.shape[:2] != (B, D)):
        raise ValueError("pscv.softargmin_bwd: grad_depth needs fp32 depth planes [B,D] or [B,D,h,w]")
    out = torch.empty((B, D, h, w, 8), dtype=dtype, device=logits.device)
    rc = _launch("softargmin_bwd", lambda: L.lib().pscv_softargmin_bwd(
        _p(logits), _p(depth), 0 if depth is None else depth.stride(0), int(depth is not None and depth.dim() == 4), _p(grad_depth),
        _p(grad_index), _p(grad_entropy), _p(out), _TORCH2PSCV[dtype], B, D, h, w, _stream()))
    L.check(rc, "pscv_softargmin_bwd")
    return out


def relu_bwd_sum(dout: torch.Tensor, out: torch.Tensor, slope: float = 0.0):
    """``relu_bwd`` that also returns the per-channel sum of the stored result (fp32 [C]): the bias gradient of a conv + bias +
    (Leaky)ReLU layer in the same pass (pscv_leaky_relu_bwd_sum)."""
    _dev(dout, out)
    _vol16(out, "relu_bwd_sum")
    if dout.shape != out.shape or dout.dtype != out.dtype:
        raise ValueError("pscv.relu_bwd_sum: dout must match out")
    Cc = out.shape[4]
    dpre = torch.empty_like(out)
    sums = torch.empty((2, Cc), dtype=torch.float32, device=out.device)
    ws = _workspace(out.device, 0)
    rc = _launch("relu_bwd_sum", lambda: L.lib().pscv_leaky_relu_bwd_sum(_p(dout), _p(out), _dt(out), out.numel() // Cc, Cc, float(slope), _p(dpre),
                                                                         _p(ws), _p(sums), _stream()))
    L.check(rc, "pscv_leaky_relu_bwd_sum")
    return dpre, sums[0]


def relu_bwd(dout: torch.Tensor, out: torch.Tensor, slope: float = 0.0) -> torch.Tensor:
    """dout * [out > 0] on 16-bit channels-last volumes (pscv_relu_bwd): backward of a ReLU applied after a residual add.
    ``slope`` > 0: dout * (out > 0 ? 1 : slope), the backward of LeakyReLU(slope) from its OUTPUT (pscv_leaky_relu_bwd)."""
    _dev(dout, out)
    _vol16(out, "relu_bwd")
    if dout.shape != out.shape or dout.dtype != out.dtype:
        raise ValueError("pscv.relu_bwd: dout must match out")
    Cc = out.shape[4]
    dpre = torch.empty_like(out)
    rc = _launch("relu_bwd", lambda: L.lib().pscv_leaky_relu_bwd(_p(dout), _p(out), _dt(out), out.numel() // Cc, Cc, float(slope), _p(dpre), _stream()))
    L.check(rc, "pscv_leaky_relu_bwd")
    return dpre


def fuse_pairs_bwd(interms: Sequence[torch.Tensor], uncerts: Sequence[torch.Tensor], grad_fused: torch.Tensor):
    """Backward of ``fuse_pairs``: ([d interm_v] 16-bit, [d uncert_v] fp32 [B,h,w]) (pscv_fuse_pairs_bwd)."""
    interms, uncerts = list(interms), list(uncerts)
    _dev(grad_fused, *interms, *uncerts)
    B, D, h, w, c = interms[0].shape
    if grad_fused.shape != interms[0].shape or grad_fused.dtype != interms[0].dtype:
        raise ValueError("pscv.fuse_pairs_bwd: grad_fused must match the pair volumes")
    n = len(interms)
    dI = [torch.empty_like(t) for t in interms]
    dU = [torch.empty((B, h, w), dtype=torch.float32, device=grad_fused.device) for _ in range(n)]
    ip = (C.c_void_p * n)(*[t.data_ptr() for t in interms])
    up = (C.c_void_p * n)(*[t.data_ptr() for t in uncerts])
    dip = (C.c_void_p * n)(*[t.data_ptr() for t in dI])
    dup = (C.c_void_p * n)(*[t.data_ptr() for t in dU])
    rc = _launch("fuse_pairs_bwd", lambda: L.lib().pscv_fuse_pairs_bwd(ip, up, n, _dt(interms[0]), _p(grad_fused), dip, dup, B, D, h, w,
                                                                      _stream()))
    L.check(rc, "pscv_fuse_pairs_bwd")
    return dI, dU


def conv3d_wgrad(p: torch.Tensor, q: torch.Tensor, *, ca: int, cb: int, stride: int, p_coff: int = 0, q_coff: int = 0) -> torch.Tensor:
    """dw[a][b][tz,ty,tx] = sum P[o,a] Q[stride*o + t - 1, b] -> fp32 [ca,cb,3,3,3] (pscv_conv3d_wgrad).
    Conv3d: p = grad of the output, q = input; ConvTranspose3d: p = input, q = grad of the output."""
    _dev(p, q)
    _vol16(p, "conv3d_wgrad")
    _vol16(q, "conv3d_wgrad")
    B, Dp, Hp, Wp, pcs = p.shape
    if q.dtype != p.dtype or tuple(q.shape[:4]) != (B, stride * Dp, stride * Hp, stride * Wp):
        raise ValueError(f"pscv.conv3d_wgrad: q must be [B,{stride}*Dp,{stride}*Hp,{stride}*Wp,*] in p's dtype")
    n = L.lib().pscv_conv3d_wgrad_workspace(B, Dp, Hp, Wp, ca, cb, stride)
    if n < 0:
        L.check(int(n), "pscv_conv3d_wgrad_workspace")
    ws = _workspace(p.device, n)
    dw = torch.empty((ca, cb, 3, 3, 3), dtype=torch.float32, device=p.device)
    rc = _launch(f"conv3d_wgrad[{ca}x{cb},s{stride}]", lambda: L.lib().pscv_conv3d_wgrad(
        _p(p), pcs, p_coff, ca, _p(q), q.shape[4], q_coff, cb, _dt(p), B, Dp, Hp, Wp, stride, _p(ws), _p(dw), 0, _stream()))
    L.check(rc, "pscv_conv3d_wgrad")
    return dw


def warp_cost_bwd(ref: Optional[torch.Tensor], srcs: Sequence[torch.Tensor], cams: torch.Tensor, depth: torch.Tensor,
                  grad_out: torch.Tensor, *, geom: int = L.GEOM_PROJ, cost: int = L.COST_VARIANCE, temp: float = 0.0,
                  ref_hw: Optional[Sequence[int]] = None, want_dtemp: bool = False):
    """Backward of ``warp_cost`` to the feature maps: returns (dref fp32 [B,h,w,C] or None, [dsrc fp32 [B,hs,ws,C]], dtemp
    fp32 [1] or None).  ``grad_out`` has the layout of the forward's output (16-bit like the features, or fp32)."""
    srcs = list(srcs)
    _dev(ref, cams, depth, grad_out, *srcs)
    B, hs, ws, Cc = srcs[0].shape
    h, w = (ref.shape[1:3] if ref is not None else ((hs, ws) if ref_hw is None else (int(ref_hw[0]), int(ref_hw[1]))))
    n = len(srcs)
    D = depth.shape[1]
    per_pixel = depth.dim() == 4
    if cost == L.COST_GROUPCORR:
        shape = (n, B, D, h, w, Cc // 4)
    elif cost == L.COST_WARP_ONLY:
        shape = (n, B, D, h, w, Cc)
    else:
        shape = (B, D, h, w, Cc)
    if tuple(grad_out.shape) != shape:
        raise ValueError(f"pscv.warp_cost_bwd: grad_out has shape {tuple(grad_out.shape)}, expected {shape}")
    dref = torch.zeros((B, h, w, Cc), dtype=torch.float32, device=srcs[0].device) if ref is not None else None
    dsrcs = [torch.zeros((B, hs, ws, Cc), dtype=torch.float32, device=srcs[0].device) for _ in srcs]
    dtemp = torch.zeros((1,), dtype=torch.float32, device=srcs[0].device) if want_dtemp else None
    sp = (C.c_void_p * n)(*[s.data_ptr() for s in srcs])
    dp = (C.c_void_p * n)(*[s.data_ptr() for s in dsrcs])
    rc = _launch(f"warp_cost_bwd[{cost}]", lambda: L.lib().pscv_warp_cost_bwd(
        _p(ref), sp, n, _p(cams), _p(depth), depth.stride(0), int(per_pixel), geom, cost, float(temp), _p(grad_out), _p(dref), dp,
        _p(dtemp), B, Cc, h, w, hs, ws, D, _dt(srcs[0]), _dt(grad_out), _stream()))
    L.check(rc, "pscv_warp_cost_bwd")
    return dref, dsrcs, dtemp


# --------------------------------------------------------------------------------------------
# loss reductions and depth-map scores (csrc/depth_gt.hip)
# --------------------------------------------------------------------------------------------
@dataclass
class LossTerm:
    """One row of the loss table (include/pscv.h, pscv_loss_terms).  ``a`` is the depth map ``d`` [b,h,w] of the ground-truth kinds
    (``gt`` / ``mask`` [b,H,W], ``interval`` [b]) or the given per-pixel loss ``l`` of the L kinds (``mask`` with as many
    elements); ``u`` is the log-uncertainty of the Bayes kinds.  Masks are bool / uint8 or fp32 holding 0 or 1."""
    kind: int
    factor: float
    a: torch.Tensor
    mask: torch.Tensor
    u: Optional[torch.Tensor] = None
    gt: Optional[torch.Tensor] = None
    interval: Optional[torch.Tensor] = None


def _f32c(t: torch.Tensor, what: str) -> torch.Tensor:
    if t.dtype != torch.float32:
        raise TypeError(f"pscv.{what}: fp32 expected, got {t.dtype}")
    return t.contiguous()


def _mask_c(m: torch.Tensor, what: str):
    """-> (contiguous mask, 1 for bytes / 0 for fp32)."""
    if m.dtype in (torch.bool, torch.uint8):
        return m.contiguous(), 1
    if m.dtype == torch.float32:
        return m.contiguous(), 0
    raise TypeError(f"pscv.{what}: a mask is bool, uint8 or fp32, got {m.dtype}")


class LossTable:
    """The parallel host arrays of a term table, with the contiguous tensors they point into kept alive.  Built once per step by
    ``loss_terms`` and handed on to ``loss_terms_bwd``."""

    def __init__(self, terms: Sequence[LossTerm]):
        terms = list(terms)
        n = len(terms)
        if n < 1:
            raise ValueError("pscv.loss_terms: no terms")
        if n > L.LOSS_MAX_TERMS:
            raise L.PscvError(f"pscv.loss_terms: {n} terms, at most {L.LOSS_MAX_TERMS} in one call")
        self.n = n
        self.a, self.u, self.gt, self.mask, self.interval = [], [], [], [], []
        kinds, u8, dims, factors = [], [], [], []
        for t, tm in enumerate(terms):
            has_gt = tm.kind in (L.LOSS_GT_PLAIN, L.LOSS_GT_BAYES)
            has_u = tm.kind in (L.LOSS_GT_BAYES, L.LOSS_L_BAYES)
            if tm.kind not in (L.LOSS_GT_PLAIN, L.LOSS_GT_BAYES, L.LOSS_L_PLAIN, L.LOSS_L_BAYES):
                raise ValueError(f"pscv.loss_terms: term {t}: unknown kind {tm.kind}")
            a = _f32c(tm.a, "loss_terms")
            mask, is_u8 = _mask_c(tm.mask, "loss_terms")
            u = _f32c(tm.u, "loss_terms") if has_u else None
            if has_u and u.numel() != a.numel():
                raise ValueError(f"pscv.loss_terms: term {t}: u has {u.numel()} elements, {a.numel()} expected")
            if has_gt:
                if a.dim() < 3 or tm.gt is None or tm.interval is None or tm.gt.dim() < 3:
                    raise ValueError(f"pscv.loss_terms: term {t}: a ground-truth kind takes d [b,h,w], gt [b,H,W], mask [b,H,W] and interval [b]")
                gt, interval = _f32c(tm.gt, "loss_terms"), _f32c(tm.interval, "loss_terms")
                b, (h, w), (H, W) = a.shape[0], a.shape[-2:], gt.shape[-2:]
                if a.numel() != b * h * w or gt.numel() != b * H * W or mask.numel() != gt.numel() or interval.numel() != b:
                    raise ValueError(f"pscv.loss_terms: term {t}: shapes d {tuple(a.shape)}, gt {tuple(gt.shape)}, mask {tuple(mask.shape)}, "
                                     f"interval {tuple(interval.shape)} do not belong together")
                dims += [b, h, w, H, W]
            else:
                gt = interval = None
                if mask.numel() != a.numel():
                    raise ValueError(f"pscv.loss_terms: term {t}: mask has {mask.numel()} elements, {a.numel()} expected")
                dims += [a.numel(), 1, 1, 0, 0]
            _dev(a, mask, u, gt, interval)
            self.a.append(a); self.u.append(u); self.gt.append(gt); self.mask.append(mask); self.interval.append(interval)
            kinds.append(int(tm.kind)); u8.append(is_u8); factors.append(float(tm.factor))
        self.device = self.a[0].device
        ptrs = lambda ts: (C.c_void_p * n)(*[None if x is None else x.data_ptr() for x in ts])
        self.c_kinds, self.c_u8 = (C.c_int * n)(*kinds), (C.c_int * n)(*u8)
        self.c_dims, self.c_factors = (C.c_long * (5 * n))(*dims), (C.c_float * n)(*factors)
        self.c_a, self.c_u, self.c_gt, self.c_mask, self.c_interval = (ptrs(x) for x in (self.a, self.u, self.gt, self.mask, self.interval))
        self.kinds = kinds

    def head(self):
        """The arguments every loss export starts with."""
        return (self.n, self.c_kinds, self.c_a, self.c_u, self.c_gt, self.c_mask, self.c_interval, self.c_u8, self.c_dims, self.c_factors)


def loss_terms(terms):
    """terms: a sequence of ``LossTerm`` (or a ``LossTable``) -> dict(loss fp32 0-dim = sum_t factor_t term_t, term fp32 [T], sums
    fp64 [T,3] = (S_l, S_u, C), norm fp32 [T], table).  Two launches whatever T is, no host wait (pscv_loss_terms)."""
    tab = terms if isinstance(terms, LossTable) else LossTable(terms)
    nbytes = L.lib().pscv_loss_terms_workspace(tab.n, tab.c_dims)
    L.check(0 if nbytes >= 0 else -1, "pscv_loss_terms_workspace")
    ws = _workspace(tab.device, (nbytes + 3) // 4)
    loss = torch.empty((), dtype=torch.float32, device=tab.device)
    term = torch.empty((tab.n,), dtype=torch.float32, device=tab.device)
    norm = torch.empty((tab.n,), dtype=torch.float32, device=tab.device)
    sums = torch.empty((tab.n, 3), dtype=torch.float64, device=tab.device)
    rc = _launch("loss_terms", lambda: L.lib().pscv_loss_terms(*tab.head(), _p(ws), _p(loss), _p(term), _p(sums), _p(norm), _stream()))
    L.check(rc, "pscv_loss_terms")
    return dict(loss=loss, term=term, sums=sums, norm=norm, table=tab)


def loss_terms_bwd(table: LossTable, norm: torch.Tensor, grad_out: torch.Tensor, want_a: Sequence[bool], want_u: Sequence[bool]):
    """Gradients of ``loss_terms``' scalar, one launch (pscv_loss_terms_bwd): ``grad_out`` fp32 0-dim / [1] on the device, ``norm``
    from the forward; ``want_a[t]`` / ``want_u[t]`` say which are written -> ([d a_t or None], [d u_t or None])."""
    _dev(norm, grad_out)
    n = table.n
    if norm.dtype != torch.float32 or norm.numel() != n or grad_out.dtype != torch.float32 or grad_out.numel() != 1:
        raise ValueError("pscv.loss_terms_bwd: norm fp32 [T] and grad_out fp32 [1] expected")
    has_u = [k in (L.LOSS_GT_BAYES, L.LOSS_L_BAYES) for k in table.kinds]
    ga = [torch.empty_like(table.a[t]) if want_a[t] else None for t in range(n)]
    gu = [torch.empty_like(table.u[t]) if (want_u[t] and has_u[t]) else None for t in range(n)]
    if all(g is None for g in ga + gu):
        return ga, gu
    pa = (C.c_void_p * n)(*[_p(g) for g in ga])
    pu = (C.c_void_p * n)(*[_p(g) for g in gu])
    rc = _launch("loss_terms_bwd", lambda: L.lib().pscv_loss_terms_bwd(*table.head(), _p(norm), _p(grad_out), pa, pu, _stream()))
    L.check(rc, "pscv_loss_terms_bwd")
    return ga, gu


def depth_metrics(est: torch.Tensor, gt: torch.Tensor, mask: torch.Tensor, step: Optional[torch.Tensor] = None, thresholds=(1, 3),
                  rel_thresholds=()):
    """The depth-map scores of models/utils.py:138-171 in one pass (pscv_depth_metrics): ``est`` [b,h,w] is upsampled bilinearly to
    ``gt``'s [b,H,W], both are divided by ``step`` [b], a pixel counts where ``mask`` > 0.5 (bool: True).  -> dict of device tensors:
    EPE, Rel, SqRel (0-dim), thres [len(thresholds)] = fraction with |e - g| > t, rel_thres [len(rel_thresholds)] = fraction with
    max(e / g, g / e) <= r -- each the mean over the batch of the per-image value --, per_image (the same keys with a leading [b])
    and sums fp64 [b,12] = (C, sum |e - g|, 4 counts, sum |e - g| / g, sum (e - g)^2 / g, 4 counts).  No host wait."""
    thr, rel = [float(t) for t in thresholds], [float(t) for t in rel_thresholds]
    MT, NS = L.METRIC_MAX_THRESH, L.METRIC_SUMS
    if len(thr) > MT or len(rel) > MT:
        raise L.PscvError(f"pscv.depth_metrics: {len(thr)} and {len(rel)} thresholds, at most {MT} of each")
    if est.dim() < 3 or gt.dim() < 3:
        raise ValueError("pscv.depth_metrics: est [b,h,w] and gt [b,H,W] expected")
    est, gt = _f32c(est, "depth_metrics"), _f32c(gt, "depth_metrics")
    mask, is_u8 = _mask_c(mask, "depth_metrics")
    step = None if step is None else _f32c(step, "depth_metrics")
    _dev(est, gt, mask, step)
    b, (h, w), (H, W) = gt.shape[0], est.shape[-2:], gt.shape[-2:]
    if est.numel() != b * h * w or gt.numel() != b * H * W or mask.numel() != gt.numel() or (step is not None and step.numel() != b):
        raise ValueError(f"pscv.depth_metrics: shapes est {tuple(est.shape)}, gt {tuple(gt.shape)}, mask {tuple(mask.shape)} do not belong together")
    nbytes = L.lib().pscv_depth_metrics_workspace(b, H, W)
    L.check(0 if nbytes >= 0 else -1, "pscv_depth_metrics_workspace")
    ws = _workspace(est.device, (nbytes + 3) // 4)
    sums = torch.empty((b, NS), dtype=torch.float64, device=est.device)
    means = torch.empty((b + 1, NS - 1), dtype=torch.float32, device=est.device)
    ta, tr = (C.c_float * MT)(*thr), (C.c_float * MT)(*rel)
    rc = _launch("depth_metrics", lambda: L.lib().pscv_depth_metrics(_p(est), _p(gt), _p(mask), is_u8, _p(step), b, h, w, H, W, ta, len(thr),
                                                                     tr, len(rel), _p(ws), _p(sums), _p(means), _stream()))
    L.check(rc, "pscv_depth_metrics")
    pick = lambda m: dict(EPE=m[..., 0], thres=m[..., 1:1 + len(thr)], Rel=m[..., 1 + MT], SqRel=m[..., 2 + MT],
                          rel_thres=m[..., 3 + MT:3 + MT + len(rel)])
    out = pick(means[b])
    out["per_image"] = pick(means[:b])
    out["sums"] = sums
    return out
