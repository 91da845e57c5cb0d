"""Store side of the brick kernel (conv3d_kernel): the descriptor instance -- one buffer descriptor each for the output and the skip
tensor per workgroup, per-lane 32-bit offsets made once, out-of-volume lanes dropped by the hardware, epilogue flags at compile
time -- which runs 16-bit outputs with c_out % 16 == 0, against the general instance (fp32 output, ragged c_out, a base that is not
8-byte aligned) and ATen, for all three kinds, both tile variants and every output-tile split, with sentinels around and inside the
output and a skip tensor read from a channel slice."""
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


S1, S2, T2 = 0, 1, 2
# (c_in, c_out, kind): the brick layers of the MVSNet U-Net, and one c_out that is no multiple of 4 (the ragged channel group)
CASES = [(16, 16, S1), (16, 32, S2), (32, 32, S1), (32, 64, S2), (64, 64, S1), (64, 32, T2), (32, 16, T2), (16, 6, S1)]
# INPUT volumes (B = 2) whose outputs cut every edge: W = 19 | 34 is no multiple of 16, D x H = 5 x 6 | 6 x 10 no multiple of a tile
IN_SHAPE = {S1: (5, 6, 19), S2: (9, 11, 37), T2: (3, 5, 17)}
B = 2
# name, ReLU before the skip add, skip, ReLU after it: what the models run (MVSNet encoder; MVSNet decoder: skip + relu(bn(deconv));
# Vis BasicBlock: relu(bn(conv) + residual))
VARIANTS = [("bn+relu", True, False, False), ("bn+relu+skip", True, True, False), ("bn+skip+relu", False, True, True)]
# name, extra channels of the output tensor, channel offset of the layer's slice, guard elements in front of the tensor
FORMS = [("slice@4", 12, 4, 64),         # out_cstride > c_out, out_coff != 0: 8-byte aligned voxels inside a wider tensor
         ("base at 4 bytes", 0, 0, 2)]    # a 16-bit tensor that is only 4-byte aligned takes the general instance's flat stores
SKIP_EXTRA, SKIP_COFF = 16, 8             # the skip tensor is a channel slice too, with its own stride and offset
SENTINEL = {2: 0x7B5A, 4: 0x7B5A7B5A}


@functools.lru_cache(maxsize=None)
def _case(cin, cout, kind):
    """Inputs and ATen references of every epilogue variant: computed once per layer, shared by both storage types (bf16-exact
    values are fp16-exact) and all tile variants, never written to.  The BatchNorm scale stays below 1 (gamma <= 1, var >= 1), so the
    error of the contraction is not amplified and the fp32 outputs keep the bars that tests/test_gpu_conv3d.py::test_conv3d_plain
    holds these layers to without an epilogue (max_abs 2e-3, rel_l2 1e-4); the skip add in fp32 adds one rounding of 2^-24."""
    g = torch.Generator().manual_seed(cin * 1000 + cout * 10 + kind)
    D, H, W = IN_SHAPE[kind]
    x = bf16_round(torch.randn(B, cin, D, H, W, generator=g))
    w = bf16_round(torch.randn((cin, cout, 3, 3, 3) if kind == T2 else (cout, cin, 3, 3, 3), generator=g) / np.sqrt(27 * cin))
    gamma, beta = torch.rand(cout, generator=g) * 0.5 + 0.5, torch.randn(cout, generator=g) * 0.3
    mean, var = torch.randn(cout, generator=g) * 0.2, torch.rand(cout, generator=g) * 0.5 + 1.0
    if kind == T2:
        y = F.conv_transpose3d(x, w, stride=2, padding=1, output_padding=1)
    else:
        y = F.conv3d(x, w, stride=1 if kind == S1 else 2, padding=1)
    y = F.batch_norm(y, mean, var, gamma, beta, training=False, eps=1e-5)
    skip = bf16_round(torch.randn(B, (cout + SKIP_EXTRA + 3) // 4 * 4, *y.shape[2:], generator=g))      # all channels of the wider skip tensor
    s = skip[:, SKIP_COFF:SKIP_COFF + cout]
    refs = {"bn+relu": F.relu(y), "bn+relu+skip": F.relu(y) + s, "bn+skip+relu": F.relu(y + s)}
    return x, w, (gamma, beta, mean, var), skip, refs


def _guarded(shape4, cs, dtype, guard):
    """[B, D, H, W, cs] inside a sentinel-filled buffer with `guard` elements in front and 64 behind; the buffer as integers."""
    es = torch.empty(0, dtype=dtype).element_size()
    n = int(np.prod(shape4)) * cs
    raw = torch.full((guard + n + 64,), SENTINEL[es], dtype=torch.int16 if es == 2 else torch.int32, device="cuda")
    return raw, raw[guard:guard + n].view(dtype).view(*shape4, cs)


def _tile_variants(nt):
    """(conv_small_tiles, conv_small_nt): the 1 x 4 x 16 tiles with the default split and every split that divides the layer's nt
    output tiles (the stride-2 kind takes the split on its 2 x 2 x 16 tiles), and the large tiles."""
    return [(1, 0)] + [(1, s) for s in (1, 2, 4) if s <= nt and nt % s == 0] + [(0, 0)]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("cin,cout,kind", CASES)
def test_brick_store_side(env, cin, cout, kind, dtype):
    """For every epilogue variant, tile variant and output form: the fp32 output (general instance) meets ATen within the bars of
    test_conv3d_plain; the 16-bit output (descriptor instance where c_out % 16 == 0 and the base is 8-byte aligned) is that fp32
    output rounded to the storage type BIT FOR BIT -- the same accumulation and epilogue arithmetic, and a store conversion that
    rounds to nearest even like torch's (values far from the fp16 range) -- and no sentinel around the tensor or in the channels beside
    the slice changes, in either output type."""
    L, ops = env
    x, w, bn, skip, refs = _case(cin, cout, kind)
    xcl, scl = ops.to_channels_last(x.cuda(), dtype), ops.to_channels_last(skip.cuda(), dtype)
    shape4 = (B, *refs["bn+relu"].shape[2:])
    nt = (cout + 15) // 16
    for vname, relu, with_skip, relu_post in VARIANTS:
        layer = ops.Conv3dLayer.build(w, kind=kind, transposed=kind == T2, device="cuda", bn=bn, relu=relu, relu_post=relu_post, dtype=dtype)
        assert layer.kind == kind
        sk = dict(skip=scl, skip_coff=SKIP_COFF) if with_skip else {}
        for small_tiles, small_nt in _tile_variants(nt):
            got32 = None
            for odt in (torch.float32, dtype):
                for fname, extra, co, guard in FORMS:
                    if odt == torch.float32 and guard != 64:
                        continue
                    cs = cout + extra + (-(cout + extra)) % 4      # (the ragged c_out = 6 in a stride of 8 or 20)
                    raw, out = _guarded(shape4, cs, odt, guard)
                    assert out.data_ptr() % 8 == (0 if guard == 64 else 4)
                    with L.tuning(conv_small_tiles=small_tiles, conv_small_nt=small_nt):
                        ops.conv3d(xcl, layer, out=out, out_coff=co, **sk)
                    torch.cuda.synchronize()
                    what = f"{cin}->{cout} kind {kind} {vname} tiles={small_tiles} nt={small_nt} {fname} {odt} ({dtype} operands)"
                    n = out.numel()
                    sent = SENTINEL[out.element_size()]
                    assert bool((raw[:guard] == sent).all()) and bool((raw[guard + n:] == sent).all()), f"guard elements overwritten: {what}"
                    body = raw[guard:guard + n].view(*shape4, cs)
                    assert bool((body[..., :co] == sent).all()) and bool((body[..., co + cout:] == sent).all()), f"channels beside the slice overwritten: {what}"
                    got = out[..., co:co + cout]
                    if odt == torch.float32:
                        got32 = got.clone()
                        check_close(f"brick vs ATen {what}", got32.permute(0, 4, 1, 2, 3).cpu(), refs[vname], max_abs=2e-3, rel_l2=1e-4)
                    else:
                        same = got.contiguous().view(torch.int16) == got32.to(dtype).view(torch.int16)
                        assert bool(same.all()), f"{what}: {int((~same).sum())} of {same.numel()} stored values differ from the rounded fp32 output"
