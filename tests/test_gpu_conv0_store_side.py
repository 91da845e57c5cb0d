"""Store side of the 32 -> 8 plane-pair depth sweep (conv3d_sweep8_kernel): per-pair buffer descriptors with per-lane 32-bit offsets,
one 16-byte store per voxel where the output voxel is 16-byte addressable (row halves exchanged between lane rows), 8-byte stores
for other 16-bit slices, float4 stores for fp32 -- against the brick kernel and ATen, with sentinels around and inside the output."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _util import bf16_round, check_close

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from wild_deep_mvs_amd import _lib as L, ops
    return L, ops


# ((D, H, W), B, 16-row tile, forced depth chunk)
GEOMETRIES = [
    ((6, 8, 16), 1, 0, 0),       # one tile, one chunk
    ((7, 12, 20), 2, 0, 0),      # odd D: the last pair's second plane is past the chunk; rows past H inside a tile; columns past W
    ((14, 24, 40), 1, 0, 6),     # three depth chunks: chunk ends inside the volume
    ((14, 24, 40), 1, 1, 6),     # the same on 16-row tiles (24 = 16 + 8: rows past H in the second tile)
]
# name, channels of the output tensor, channel offset of the layer's slice, fp32 output, guard elements in front of the tensor
FORMS = [
    ("f32", 8, 0, True, 64),
    ("plain", 8, 0, False, 64),          # 16-byte stores (with the BN + ReLU variant: the compile-time instance MVSNet's conv0 runs)
    ("slice@8", 24, 8, False, 64),       # 16-byte stores at a 48-byte voxel stride
    ("slice@4", 16, 4, False, 64),       # voxel not 16-byte aligned: 8-byte stores
    ("plain, base at 8 bytes", 8, 0, False, 4),   # the tensor itself is only 8-byte aligned: 8-byte stores
]
# name, residual, ReLU after the residual
VARIANTS = [("bn+relu", False, False), ("bn+relu+skip+relu", True, True)]
SENTINEL = {2: 0x7B5A, 4: 0x7B5A7B5A}


@functools.lru_cache(maxsize=None)
def _case(shape, B):
    """Inputs and the ATen references of both epilogue variants: computed once per geometry, shared, never written to.
    The input is random ON PURPOSE: the two pixel rows of a wave differ, so an exchange that pairs the wrong rows or halves in the
    16-byte store already fails the comparison with the brick kernel.  Do not replace it by a constant."""
    g = torch.Generator().manual_seed(sum(shape) + B)
    D, H, W = shape
    x = bf16_round(torch.randn(B, 32, D, H, W, generator=g))
    w = bf16_round(torch.randn(8, 32, 3, 3, 3, generator=g) / np.sqrt(27 * 32))
    gamma, beta = torch.rand(8, generator=g) + 0.5, torch.randn(8, generator=g) * 0.3
    mean, var = torch.randn(8, generator=g) * 0.2, torch.rand(8, generator=g) + 0.5
    skip = bf16_round(torch.randn(B, 8, D, H, W, generator=g))
    y = F.relu(F.batch_norm(F.conv3d(x, w, padding=1), mean, var, gamma, beta, training=False, eps=1e-5))
    refs = {"bn+relu": y, "bn+relu+skip+relu": F.relu(y + skip)}
    return x, w, (gamma, beta, mean, var), skip, refs


def _guarded(B, D, H, W, cs, dtype, guard):
    """[B, D, H, W, cs] inside a sentinel-filled buffer with `guard` elements in front and 64 behind; the buffer as integers.
    (Device allocations are at least 256-byte aligned: the tensor starts `guard` elements behind such a boundary.)"""
    es = torch.empty(0, dtype=dtype).element_size()
    n = B * D * H * W * cs
    raw = torch.full((guard + n + 64,), SENTINEL[es], dtype=torch.int16 if es == 2 else torch.int32, device="cuda")
    return raw, raw[guard:guard + n].view(dtype).view(B, D, H, W, cs)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("shape,B,th16,dc", GEOMETRIES)
def test_sweep_store_forms_match_brick_kernel_and_aten(env, shape, B, th16, dc, dtype):
    """Every output form of the plane-pair sweep, for both epilogue variants.  The fp32 form meets the bars of
    test_gpu_conv3d.py::test_sweep_kernel_matches_brick_kernel_and_aten (ATen: max_abs 3e-3, rel_l2 2e-4; brick kernel: max_abs 1e-4).
    Every 16-bit form must be the fp32 form rounded to the storage type BIT FOR BIT: the accumulation and the epilogue are the same
    instructions and the store conversion rounds to nearest even like torch's (values far from the fp16 range), so the 16-bit forms
    inherit those bars with nothing added but the storage rounding.  No sentinel around the tensor or in the channels beside the slice
    may change."""
    L, ops = env
    D, H, W = shape
    x, w, bn, skip, refs = _case(shape, B)
    xcl, scl = ops.to_channels_last(x.cuda(), dtype), ops.to_channels_last(skip.cuda(), dtype)
    for vname, with_skip, relu_post in VARIANTS:
        layers = {}
        for use in (True, False):
            ops.USE_SWEEP_KERNEL = use
            try:
                layers[use] = ops.Conv3dLayer.build(w, kind=L.CONV_S1, device="cuda", bn=bn, relu=True, relu_post=relu_post, dtype=dtype)
            finally:
                ops.USE_SWEEP_KERNEL = True
            assert layers[use].kind == (L.CONV_S1P8 if use else L.CONV_S1)
        sk = scl if with_skip else None
        brick = ops.conv3d(xcl, layers[False], skip=sk, out_dtype=torch.float32)
        got32 = None
        for fname, cs, co, f32, guard in FORMS:
            odt = torch.float32 if f32 else dtype
            raw, out = _guarded(B, D, H, W, cs, odt, guard)
            assert out.data_ptr() % 16 == (0 if guard % 8 == 0 else 8)
            with L.tuning(sweep_th16=th16, sweep_dc=dc):
                ops.conv3d(xcl, layers[True], skip=sk, out=out, out_coff=co)
            torch.cuda.synchronize()
            what = f"{fname} {vname} {shape} B={B} th16={th16} dc={dc} {dtype}"
            n = out.numel()
            sent = SENTINEL[out.element_size()]
            assert bool((raw[:guard] == sent).all()) and bool((raw[guard + n:] == sent).all()), f"guard elements overwritten: {what}"
            body = raw[guard:guard + n].view(B, D, H, W, cs)
            assert bool((body[..., :co] == sent).all()) and bool((body[..., co + 8:] == sent).all()), f"channels beside the slice overwritten: {what}"
            got = out[..., co:co + 8]
            if f32:
                got32 = got.clone()
                g5 = got32.permute(0, 4, 1, 2, 3).cpu()
                check_close(f"sweep vs ATen {what}", g5, refs[vname], max_abs=3e-3, rel_l2=2e-4)
                check_close(f"sweep vs brick {what}", g5, brick.permute(0, 4, 1, 2, 3).cpu(), max_abs=1e-4)
            else:
                want = got32.to(dtype)
                same = got.contiguous().view(torch.int16) == want.view(torch.int16)
                assert bool(same.all()), f"{what}: {int((~same).sum())} of {same.numel()} stored values differ from the rounded fp32 output"
