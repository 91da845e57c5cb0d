"""pscv_conv3d / pscv_conv3d_cat2 (ops.conv3d) held to the float64 reference of tests/_conv3d_ref.py: every instantiation the host can
select -- the 27 brick instantiations with both tile variants and every output-tile split, the tall tile, the persistent wide kernel,
the plane-pair, kd-in-rows, narrow and stride-2 depth sweeps, the parity-pair deconv and both variants of the 1-channel head -- in
fp16 and bf16, at the smallest sizes at which each can go wrong (the case table lives in _conv3d_ref.py; tests/test_conv3d_ref_cpu.py
checks it against the dispatch code and checks the operands without a GPU).

What is asserted:
  * fp32 outputs, per element: |got - ref| <= c 2^-24 U with U = |scale| (|w| conv |x|) + |bias| + |skip| (``BOUND``: 4 x the worst
    ratio measured over all cases of a kernel and storage type on an MI355X, rounded up; DESIGN.md section 5 holds the table), never
    above K + 3 (the worst case of an fp32 sum of K exact products in any order plus the epilogue's roundings) and never looser in
    max-abs than the bars of tests/test_gpu_conv3d.py (2e-3 brick, 3e-3 the others);
  * 16-bit outputs equal ``round16`` of the fp32 output of the same operands bit for bit: dense, as the channel slice at offset 8 of
    NaN-filled wider tensors (input, skip and output; the brick kernel's descriptor instance where c_out % 16 == 0) and at offsets of 4
    (the brick kernel's plain instance: its output base is only 4-byte aligned there);
  * every output starts as NaN: a voxel, plane or channel group that is not written shows, and the channels beside a slice keep
    their bits; the NaN beside the input and skip slices stays out;
  * instantiations documented as bit-identical are: wide = brick, tall = 4 x 4 x 16, cat2 = concatenated input, the 1-channel
    head's sweep = its brick variant (fp32);
  * the epilogue algebra (finite, -inf and ignored floors, PRE | POST, missing scale or bias), non-finite values beside and through
    the MFMA, and fp16 saturation, per kernel (``EDGE_CASES``);
  * the fused kernels (tail sweep, residual block, prob + softargmin) give the bits of their two-launch paths on such operands."""
import dataclasses
import json
import os

import pytest
import torch

import _conv3d_ref as R

pytestmark = pytest.mark.gpu

# (kernel, storage type): bound c in units of 2^-24 U.    worst measured ratio (MI355X) and the case that gave it    4 x worst
BOUND = {
    ("brick", "fp16"): 9,                                # 2.237 (16 -> 16 T2, 1 x 4 x 16 tiles, 2 x 2 x 5 x 17, saturation)   8.9
    ("brick", "bf16"): 11,                               # 2.510 (64 -> 32 S1, 4 x 4 x 16 tiles, 3 x 5 x 5 x 17)              10.0
    ("wide", "fp16"): 9,                                 # 2.170 (32 -> 64, the long volume, rows 161..172)                  8.7
    ("wide", "bf16"): 7,                                 # 1.734 (32 -> 64, the long volume, rows 82..93)                    6.9
    ("pair", "fp16"): 7,                                 # 1.655 (16-row tiles, 2 x 9 x 17 x 17)                             6.6
    ("pair", "bf16"): 8,                                 # 1.835 (transposed, 2 x 9 x 9 x 17)                                7.3
    ("kdm", "fp16"): 7,                                  # 1.709 (sweep_kdm 1, pd 2, 2 x 17 x 9 x 17, floor ignored)         6.8
    ("kdm", "bf16"): 7,                                  # 1.714 (sweep_kdm 2, pd 2, 2 x 9 x 9 x 17)                         6.9
    ("narrow", "fp16"): 9,                               # 2.008 (16 -> 16, pd 3, 3 x 17 x 9 x 17)                           8.0
    ("narrow", "bf16"): 9,                               # 2.018 (cat2 -> 8, 3 x 17 x 9 x 17)                                8.1
    ("s2sweep", "fp16"): 8,                              # 1.898 (8 -> 32, 3 x 21 x 17 x 33)                                 7.6
    ("s2sweep", "bf16"): 9,                              # 2.030 (8 -> 32, 3 x 21 x 17 x 33)                                 8.1
    ("t2p8", "fp16"): 8,                                 # 1.858 (2 x 3 x 5 x 17, no bias)                                   7.4
    ("t2p8", "bf16"): 7,                                 # 1.713 (3 x 3 x 5 x 17, with skip)                                 6.9
    ("c1", "fp16"): 6,                                   # 1.351 (8 -> 1, 2 x 7 x 5 x 33, saturation)                        5.4
    ("c1", "bf16"): 5,                                   # 1.200 (16 -> 1, 3 x 7 x 5 x 33)                                   4.8
    ("c1sweep", "fp16"): 5,                              # 1.194 (2 x 37 x 5 x 33)                                           4.8
    ("c1sweep", "bf16"): 4,                              # 0.866 (2 x 37 x 5 x 33)                                           3.5
}
ABS_BAR = {"brick": 2e-3}                                   # max |got - ref| of today's tests (3e-3 for every other kernel)
WORST, WORST_AT = {}, {}
NAN, INF = float("nan"), float("inf")
F32 = torch.float32


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from wild_deep_mvs_amd import _lib as L, ops
    L.lib()
    yield L, ops
    print("\n[parity] conv3d ref: worst |got - ref| / (2^-24 U) per kernel and storage type", flush=True)
    for (kern, dt), v in sorted(WORST.items()):
        print(f"[parity] conv3d ref worst {kern:8s} {dt:5s} {v:.3f} at {WORST_AT[(kern, dt)]} (bound {BOUND[(kern, dt)]})", flush=True)
    path = os.environ.get("PSCV_CONV3D_ERR_TABLE")
    if path:
        with open(path, "w") as fh:
            json.dump({f"{kern}/{dt}": [v, WORST_AT[(kern, dt)]] for (kern, dt), v in sorted(WORST.items())}, fh, indent=1)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def same_stored(a, b):
    """Equal bits, except that any NaN matches any NaN (an MFMA's or an inf - inf NaN need not carry torch's payload)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(_bits(a)[~na], _bits(b)[~nb])


def compare32(tag, kern, dt, got, ref_y, U, K, *, mask=None, abs_bar=True):
    """fp32 ``got`` against the float64 ``ref_y`` on the elements of ``mask`` (all): NaN and inf exactly where the reference has them,
    exact equality where the error unit is not finite (an inf bias or skip element), the rest within the bound."""
    got = got.detach().double().cpu()
    assert got.shape == ref_y.shape, (tag, got.shape, ref_y.shape)
    if mask is not None:
        got, ref_y, U = got[mask], ref_y[mask], U[mask]
    nan = torch.isnan(ref_y)
    assert torch.equal(torch.isnan(got), nan), f"{tag}: NaN at {int(torch.isnan(got).sum())} elements, reference at {int(nan.sum())}"
    inf = torch.isinf(ref_y)
    assert torch.equal(got[inf], ref_y[inf]), f"{tag}: inf elements differ"
    exact = ~(nan | inf) & ~torch.isfinite(U)
    assert torch.equal(got[exact], ref_y[exact]), f"{tag}: elements behind an infinite bias / skip value differ"
    fin = ~(nan | inf | exact)
    err = (got - ref_y).abs()[fin]
    ratio = float((err / (2.0 ** -24 * U[fin])).max())
    if ratio > WORST.get((kern, dt), -1.0):
        WORST[(kern, dt)], WORST_AT[(kern, dt)] = ratio, tag
    bound = min(BOUND[(kern, dt)], K + 3)
    line = f"[parity] conv3d ref {tag}: max err / (2^-24 U) = {ratio:.3f} (bound {bound}, K + 3 = {K + 3}) max_abs={float(err.max()):.3e}"
    print(line, flush=True)
    assert ratio <= bound, line
    if abs_bar:
        assert float(err.max()) <= ABS_BAR.get(kern, 3e-3), line


def _wide(t, width, off, fill=NAN):
    """``t`` [..., c] as channels [off, off + c) of a new [..., width] tensor whose other channels hold ``fill``."""
    out = torch.full(t.shape[:-1] + (width,), fill, dtype=t.dtype)
    out[..., off:off + t.shape[-1]] = t
    return out


def _kind(L, c):
    if c.kernel in ("pair", "kdm", "narrow"):
        return L.CONV_S1P8
    if c.kernel == "t2p8":
        return L.CONV_T2P8
    if c.kernel in ("c1", "c1sweep"):
        return L.CONV_S1C1
    return {"S1": L.CONV_S1, "S2": L.CONV_S2, "T2": L.CONV_T2}[c.kind]


def _check_fold(layer, o):
    """The layer's folded epilogue vectors (Conv3dLayer.build on the device) become the reference's operands.  They are the CPU fold
    (_conv2d_ref.fold_bn, the operation order of Conv3dLayer.build) up to the device's fp32 sqrt and division, within 2 ulp of the
    correctly rounded ones: 1e-6 relative on the scale, 1e-6 of the O(1) terms beta and mean * scale on the bias."""
    for got, want in ((layer.scale, o["scale"]), (layer.bias, o["bias"])):
        assert (got is None) == (want is None)
        if got is not None:
            torch.testing.assert_close(got.cpu(), want, rtol=1e-6, atol=1e-6)
    o["scale"] = None if layer.scale is None else layer.scale.cpu()
    o["bias"] = None if layer.bias is None else layer.bias.cpu()


# output forms: (name, input channel offset, skip width - c_out and offset, output width - c_out and offset, 4-byte aligned output base)
DENSE = ("dense", 0, 0, 0, 0, 0, False)
SLICE8 = ("slice@8", 8, 16, 8, 24, 8, False)
SLICE4 = ("slice@4", 8, 8, 4, 8, 4, True)


class Launch:
    """One (row, size, storage type): operands, the layer, the knobs, launches in every output form and their references."""

    def __init__(self, env, c, dtype, B, D, H, W, epilogue, size_knobs, seed=0):
        self.L, self.ops = env
        self.c, self.dtype = c, dtype
        self.o = R.make_operands(c, dtype, B, D, H, W, epilogue=epilogue, seed=seed)
        ops = self.ops
        saved = ops.USE_SWEEP_KERNEL, ops.SWEEP16
        ops.USE_SWEEP_KERNEL, ops.SWEEP16 = c.sweep
        try:
            o = self.o
            self.layer = ops.Conv3dLayer.build(o["w"], kind={"S1": self.L.CONV_S1, "S2": self.L.CONV_S2, "T2": self.L.CONV_T2}[c.kind],
                                               transposed=c.transposed, device="cuda", bn=o["bn"], conv_bias=o["conv_bias"], relu=o["relu_pre"],
                                               relu_post=o["relu_post"], dtype=dtype)
        finally:
            ops.USE_SWEEP_KERNEL, ops.SWEEP16 = saved
        assert self.layer.kind == _kind(self.L, c) and (self.layer.c_in, self.layer.c_out) == (c.c_in, c.c_out)
        _check_fold(self.layer, self.o)
        self.knobs = R.resolve_knobs(c, B, D, H, W, size_knobs)
        self.out_shape = (B,) + R.out_dhw(c.kind, D, H, W)

    def variant(self, *, epi, floor=None, **vec):
        """A copy whose layer has these epilogue flags, this floor and -- where given -- scale / bias (None: the vector is absent)."""
        v = Launch.__new__(Launch)
        v.__dict__.update(self.__dict__)
        v.o = dict(self.o)
        for k, t in vec.items():
            v.o[k] = t
        v.o["relu_pre"], v.o["relu_post"], v.o["floor"] = bool(epi & self.L.EPI_RELU_PRE), bool(epi & self.L.EPI_RELU_POST), floor
        dev = lambda t: None if t is None else t.float().cuda().contiguous()
        v.layer = dataclasses.replace(self.layer, epi=epi, scale=dev(v.o["scale"]), bias=dev(v.o["bias"]), floor=dev(floor))
        return v

    def ref(self, with_skip):
        return R.reference(self.c, self.o, with_skip=with_skip, floor=self.o["floor"])

    def run(self, out_dtype, form=DENSE, *, skip=False, cat=False):
        """One launch into a NaN-filled output; returns the whole output tensor [B,Do,Ho,Wo,width] (on the GPU)."""
        _, in_off, sk_extra, sk_off, out_extra, out_off, odd_base = form
        c, o, ops = self.c, self.o, self.ops
        co = c.c_out
        n = 1
        for s in self.out_shape:
            n *= s
        width = co + out_extra
        guard = 2 if (odd_base and c.kernel == "brick" and out_dtype != F32) else 0      # (2 elements = 4 bytes: conv3d_kernel's plain instance)
        raw = torch.full((guard + n * width,), NAN, dtype=out_dtype, device="cuda")
        out = raw[guard:].view(*self.out_shape, width)
        assert out.data_ptr() % 8 == 2 * guard
        sk = None if not skip else (_wide(o["skip"], co + sk_extra, sk_off) if sk_extra else o["skip"]).cuda()
        kw = dict(skip=sk, skip_coff=sk_off if skip else 0, out=out, out_coff=out_off)
        x = o["x"]
        if c.cat2 and not cat:
            a, b = x[..., :8], x[..., 8:]
            if in_off:
                a, b, kw["in_coff"], kw["x2_coff"] = _wide(a, 24, 16), _wide(b, 16, 0), 16, 0
            ops.conv3d(a.contiguous().cuda(), self.layer, x2=b.contiguous().cuda(), **kw)
        else:
            if in_off:
                x, kw["in_coff"] = _wide(x, c.c_in + 2 * in_off, in_off), in_off
            ops.conv3d(x.cuda(), self.layer, **kw)
        torch.cuda.synchronize()
        return out


def check_forms(tag, run, dt):
    """fp32 without and with a skip against float64 (the second one through slices of NaN-filled wider tensors), then the 16-bit
    forms against round16 of those fp32 outputs."""
    c, dtype = run.c, run.dtype
    kern, co = c.kernel, c.c_out
    r = run.ref(False)
    a = run.run(F32).cpu()
    compare32(f"{tag} fp32", kern, dt, a, r.y, r.U, r.K)
    rs = run.ref(True)
    a_s = run.run(F32, SLICE8, skip=True).cpu()
    assert same_bits(a_s[..., :8], torch.full_like(a_s[..., :8], NAN)) and same_bits(a_s[..., 8 + co:], torch.full_like(a_s[..., 8 + co:], NAN)), \
        f"{tag}: channels beside the fp32 output slice changed"
    a_s = a_s[..., 8:8 + co]
    compare32(f"{tag} fp32+skip", kern, dt, a_s, rs.y, rs.U, rs.K)
    assert same_bits(run.run(dtype).cpu(), R.round16(a, dtype)), f"{tag}: the dense 16-bit output is not the rounded fp32 output"
    want = R.round16(a_s, dtype)
    for form in (SLICE8, SLICE4):
        got = run.run(dtype, form, skip=True).cpu()
        assert same_bits(got, _wide(want, co + form[4], form[5])), f"{tag}: 16-bit {form[0]} is not the rounded fp32 output inside NaN-filled channels"
    return a, a_s


def _twin_knobs(c):
    return dict(c.twin)


@pytest.mark.parametrize("dt", list(R.DTYPES))
@pytest.mark.parametrize("c", R.CASES, ids=lambda c: c.name)
def test_every_instantiation_equals_float64_reference(env, c, dt):
    """Every row of the case table at each of its sizes (1 x 1 x 1; two tiles per axis, the last one voxel thick; for the sweeps a
    chunk in which the plane ring wraps twice and a seam in front of a one-plane chunk), B = 2 and 3 alternating, the epilogues
    rotating over BN + ReLU + skip, BN + skip + post-ReLU, bias only and none with about half of the BatchNorm scales negative."""
    L, ops = env
    dtype = R.DTYPES[dt]
    ci = R.CASES.index(c)
    for si, (D, H, W, kn) in enumerate(c.sizes):
        B = R.batch_of(si)
        run = Launch(env, c, dtype, B, D, H, W, R.epilogue_of(ci, si), kn)
        tag = f"{c.name} {dt} {B}x{D}x{H}x{W}"
        with L.tuning(**run.knobs):
            a, a_s = check_forms(tag, run, dt)
            h_s = run.run(dtype, SLICE8, skip=True).cpu()
        if c.twin is not None and not c.twin32:
            with L.tuning(**_twin_knobs(c)):
                b, b_s = run.run(F32).cpu(), run.run(F32, SLICE8, skip=True).cpu()[..., 8:8 + c.c_out]
                g_s = run.run(dtype, SLICE8, skip=True).cpu()
            assert same_bits(a, b) and same_bits(a_s, b_s), f"{tag}: fp32 bits differ from {c.twin}"
            assert same_bits(h_s, g_s), f"{tag}: 16-bit bits differ from {c.twin}"
        if c.cat2:
            with L.tuning(**run.knobs):
                b, b_s = run.run(F32, cat=True).cpu(), run.run(F32, SLICE8, skip=True, cat=True).cpu()[..., 8:8 + c.c_out]
                g_s = run.run(dtype, SLICE8, skip=True, cat=True).cpu()
            assert same_bits(a, b) and same_bits(a_s, b_s) and same_bits(h_s, g_s), f"{tag}: two input tensors differ from the concatenated one"


@pytest.mark.parametrize("dt", list(R.DTYPES))
def test_one_channel_sweep_equals_its_brick_variant_bit_for_bit(env, dt):
    """The depth-sweep variant of the 1-channel head (c1_sweep = 2) against its brick variant (c1_sweep = 0), fp32 outputs without
    and with a skip, at every size of the row: the same bits.

    Both kernels sum an output's 18 MFMA steps as two chains of 9 (the two plane sets of a lane group) that they add at the end.
    (conv3d_c1_kernel used to run one chain of 18: on that library 41 .. 63 % of the fp32 values of the sizes beyond 1 x 1 x 1
    differed from the sweep's, by at most 1.7 units of 2^-24 U, each variant within its bound of the float64 reference.)"""
    L, ops = env
    c = R.BY_NAME["c1in8sweep"]
    assert c.twin32 and c.twin == {"c1_sweep": 0}
    ci = R.CASES.index(c)
    bad = []
    for si, (D, H, W, kn) in enumerate(c.sizes):
        B = R.batch_of(si)
        run = Launch(env, c, R.DTYPES[dt], B, D, H, W, R.epilogue_of(ci, si), kn)
        with L.tuning(**run.knobs):
            a, a_s = run.run(F32).cpu(), run.run(F32, SLICE8, skip=True).cpu()[..., 8:9]
        with L.tuning(**c.twin):
            b, b_s = run.run(F32).cpu(), run.run(F32, SLICE8, skip=True).cpu()[..., 8:9]
        for name, x, y, r in (("fp32", a, b, run.ref(False)), ("fp32+skip", a_s, b_s, run.ref(True))):
            ne = int((_bits(x) != _bits(y)).sum())
            worst = float(((x.double() - y.double()).abs() / (2.0 ** -24 * r.U)).max())
            print(f"[parity] conv3d ref c1 sweep vs brick variant {dt} {B}x{D}x{H}x{W} {name}: {ne} of {x.numel()} values differ, "
                  f"max |diff| / (2^-24 U) = {worst:.3f}", flush=True)
            if ne:
                bad.append((B, D, H, W, name, ne, x.numel(), round(worst, 3)))
    assert not bad, f"c1 sweep differs from its brick variant: {bad}"


@pytest.mark.parametrize("dt", list(R.DTYPES))
@pytest.mark.parametrize("c", R.WIDE_CASES, ids=lambda c: c.name)
def test_wide_kernel_loops_over_tiles(env, c, dt):
    """The long volume of _conv3d_ref.long_volume (1 x 13 x H x 33 with at least 2 grid + 3 tiles, grid = n_cu & ~7: H = 173 and 528
    tiles on 256 CUs): every persistent workgroup of conv3d_widep_kernel takes a second tile and some a third, flipping the weight
    double buffer for a new tile.  The whole output equals the brick kernel's bit for bit (fp32 and 16-bit slice, with a skip) and --
    at least 512 tiles -- the default knob's; three 12-row bands are held to float64."""
    L, ops = env
    dtype = R.DTYPES[dt]
    B, D, H, W, grid, tiles = R.long_volume(torch.cuda.get_device_properties(0).multi_processor_count)
    assert tiles >= 2 * grid + 3 and tiles >= 512
    run = Launch(env, c, dtype, B, D, H, W, R.epilogue_of(R.CASES.index(c), 1), {})
    res = {}
    arms = [("wide", {"conv_wide": 2}), ("brick", c.twin)] + ([("default", {"conv_wide": 1})] if c.c_in == 64 else [])      # (32 inputs: forced only)
    for name, kn in arms:
        with L.tuning(**kn):
            res[name] = (run.run(F32, SLICE8, skip=True).cpu(), run.run(dtype, SLICE8, skip=True).cpu())
    for name, _ in arms[1:]:
        for form, x, y in zip(("fp32", "16-bit"), res[name], res["wide"]):
            ne = int((_bits(x) != _bits(y)).sum())
            assert ne == 0, f"{c.name} {dt}: {ne} {form} values of conv_wide = 2 differ from the {name} launch"
    co = c.c_out
    f32 = res["wide"][0][..., 8:8 + co]
    assert same_bits(res["wide"][1], _wide(R.round16(f32, dtype), co + 24, 8))
    o = run.o
    for h0 in (0, (H // 2) // 4 * 4 - 2, H - 12):
        lo, hi = max(h0 - 1, 0), min(h0 + 13, H)
        r = R.conv3d(o["x"][:, :, lo:hi], o["w"], kind="S1", transposed=c.transposed, scale=o["scale"], bias=o["bias"], skip=o["skip"][:, :, lo:hi],
                     relu_pre=o["relu_pre"], relu_post=o["relu_post"], K=R.k_terms(c))
        rows = slice(h0 - lo, h0 - lo + 12)
        compare32(f"{c.name} {dt} 1x{D}x{H}x{W} rows {h0}..{h0 + 11}", "wide", dt, f32[:, :, h0:h0 + 12], r.y[:, :, rows], r.U[:, :, rows], r.K)


def _edge_launch(env, c, dt, epilogue="bn_relu_skip"):
    B, D, H, W, kn = R.edge_size(c)
    return Launch(env, c, R.DTYPES[dt], B, D, H, W, epilogue, kn), f"{c.name} {dt} {B}x{D}x{H}x{W}"


def _check_16bit(tag, run, a_s, compare=same_bits):
    co = run.c.c_out
    want = R.round16(a_s, run.dtype)
    for form in (SLICE8, SLICE4):
        got = run.run(run.dtype, form, skip=True).cpu()
        assert compare(got, _wide(want, co + form[4], form[5])), f"{tag}: 16-bit {form[0]} is not the rounded fp32 output"
    return want


@pytest.mark.parametrize("dt", list(R.DTYPES))
@pytest.mark.parametrize("c", R.EDGE_CASES, ids=lambda c: c.name)
def test_floors_and_epilogue_flags(env, c, dt):
    """floor = [-0.5, 0.25, -inf, 0, ...] over the channels, negative scales: applied with RELU_PRE; the same tensor ignored without
    RELU_PRE (alone and with RELU_POST + skip); RELU_PRE | RELU_POST + skip; a layer without a scale (bias only) and one without a
    bias (scale only) -- on the branching epilogues (brick, sweeps) and the clamp forms (t2p8, stride-2 sweep, 1-channel head)."""
    L, ops = env
    base, tag = _edge_launch(env, c, dt)
    PRE, POST = L.EPI_RELU_PRE, L.EPI_RELU_POST
    floor = R.cycled_floor(c.c_out)
    o = base.o
    variants = [("floor applied", dict(epi=PRE)), ("floor ignored", dict(epi=0)), ("floor ignored, post", dict(epi=POST)),
                ("pre|post", dict(epi=PRE | POST)), ("no scale", dict(epi=PRE, scale=None)), ("no bias", dict(epi=PRE | POST, bias=None))]
    with L.tuning(**base.knobs):
        for name, kw in variants:
            run = base.variant(floor=floor, **kw)
            r = run.ref(True)
            if kw["epi"] & PRE:          # the floors bite: each of the three finite floors is the value of some element before the skip add
                pre = R.reference(c, run.o, with_skip=False, floor=floor, relu_post=False).y
                assert all(bool((pre[..., k::4] == f).any()) for k, f in enumerate(R.CYCLED_FLOORS) if f != -INF and k < c.c_out)
            a_s = run.run(F32, SLICE8, skip=True).cpu()[..., 8:8 + c.c_out]
            compare32(f"{tag} {name}", c.kernel, dt, a_s, r.y, r.U, r.K)
            r0 = run.ref(False)
            compare32(f"{tag} {name}, no skip", c.kernel, dt, run.run(F32).cpu(), r0.y, r0.U, r0.K)
            _check_16bit(f"{tag} {name}", run, a_s)
    assert o is base.o and base.o["floor"] is None


@pytest.mark.parametrize("dt", list(R.DTYPES))
@pytest.mark.parametrize("c", R.EDGE_CASES, ids=lambda c: c.name)
def test_non_finite_values_beside_the_mfma(env, c, dt):
    """-inf, +inf and NaN at three voxels of the skip tensor and -inf as the bias of the last channel, under RELU_PRE (cycled floors),
    RELU_POST and both: the fp32 output has 0, the floor, +inf or NaN exactly where the reference has them (relu(-inf) = 0), and the
    16-bit outputs are round16 of it: +inf is stored as 65504 in fp16 and as inf in bf16, no NaN becomes a number."""
    L, ops = env
    base, tag = _edge_launch(env, c, dt)
    PRE, POST = L.EPI_RELU_PRE, L.EPI_RELU_POST
    base.o["skip"] = base.o["skip"].clone()
    vox = R.skip_voxels(c, base.o["skip"].shape)
    R.poison_skip_and_bias(c, base.o, vox)
    floor = R.cycled_floor(c.c_out)
    big = R.F16_MAX if base.dtype == torch.float16 else INF
    with L.tuning(**base.knobs):
        for epi in (PRE, POST, PRE | POST):
            run = base.variant(epi=epi, floor=floor, bias=base.o["bias"])
            r = run.ref(True)
            assert bool(torch.isnan(r.y[vox[2]]).all()) and bool((r.y[vox[1]] == INF).any()) and bool((r.y[vox[0]] == (0.0 if epi & POST else -INF)).all())
            a_s = run.run(F32, SLICE8, skip=True).cpu()[..., 8:8 + c.c_out]
            compare32(f"{tag} non-finite skip / bias, epi {epi}", c.kernel, dt, a_s, r.y, r.U, r.K)
            want = _check_16bit(f"{tag} non-finite skip / bias, epi {epi}", run, a_s, compare=same_stored)
            pinf = r.y[vox[1]] == INF
            assert bool((want[vox[1]][pinf].double() == big).all()) and bool(torch.isnan(want[vox[2]]).all())
            assert bool((want[vox[0]].double() == (0.0 if epi & POST else -big)).all())


def _reach(c, vox_out, p):
    """Per axis, how far output voxels (rows of [n, 4] = b, d, h, w) lie from the footprint centre of input voxel p (b, d, h, w)."""
    d = []
    for ax in (1, 2, 3):
        o = vox_out[:, ax]
        d.append(((o - p[ax]) if c.kind == "S1" else (2 * o - p[ax]) if c.kind == "S2" else (o // 2 - p[ax])).abs())
    return d


@pytest.mark.parametrize("dt", list(R.DTYPES))
@pytest.mark.parametrize("relu", [True, False], ids=["relu", "linear"])
@pytest.mark.parametrize("c", R.EDGE_CASES, ids=lambda c: c.name)
def test_non_finite_values_through_the_mfma(env, c, relu, dt):
    """+inf and NaN at two input voxels (different batch items).  Inside the reference's footprint of each: NaN stays NaN; +-inf stays
    +-inf and relu(-inf) + skip stays that number -- or becomes NaN where the kernel's reduction also meets the voxel with a
    zero-weight entry (_conv3d_ref.inf_may_turn_nan: the k padding of the brick and stride-2 kernels, the repeated plane of the
    16 -> 16 sweep).  Outside it the kernels that pad their MFMA rows with zero weights may add NaN (never inf, never a number where
    the reference has none): at most ``halo`` <= 3 depth planes further, inside the 3 x 3 (h, w) footprint, and no more elements than
    the reference's own footprint holds.  Everywhere else the numeric bound holds.  The 16-bit outputs are round16 of the fp32 one."""
    L, ops = env
    base, tag = _edge_launch(env, c, dt)
    tag += " relu" if relu else " linear"
    B, D, H, W, _ = R.edge_size(c)
    p_inf, p_nan = R.nonfinite_voxels(c, D, H, W)
    base.o["x"] = base.o["x"].clone()
    base.o["x"][p_inf][1 % c.c_in], base.o["x"][p_nan][c.c_in - 1] = INF, NAN
    run = base.variant(epi=L.EPI_RELU_PRE if relu else 0)
    r = run.ref(True)
    nf = R.acc_nonfinite(run.o["x"], run.o["w"], kind=c.kind, transposed=c.transposed)          # [B,Do,Ho,Wo]
    with L.tuning(**run.knobs):
        got = run.run(F32, SLICE8, skip=True).cpu()[..., 8:8 + c.c_out]
        # inside the reference's footprint
        g, y = got.double()[nf], r.y[nf]
        gnan, ynan = torch.isnan(g), torch.isnan(y)
        assert bool((gnan | ~ynan).all()), f"{tag}: {int((ynan & ~gnan).sum())} NaN elements of the reference are numbers here"
        other = ~ynan & ~gnan
        assert torch.equal(g[other], y[other]), f"{tag}: inf / relu(-inf) elements differ"
        lenient = R.inf_may_turn_nan(c)
        assert lenient or torch.equal(gnan, ynan), f"{tag}: {int((gnan & ~ynan).sum())} inf elements became NaN in a kernel without zero-weight entries"
        # outside it
        extra = ~torch.isfinite(got) & ~nf.unsqueeze(-1)
        assert not bool(torch.isinf(got[extra]).any())
        halo = min(c.halo, R.HALO_MAX)
        ev = torch.nonzero(extra.any(-1))
        assert halo > 0 or c.kernel == "t2p8" or len(ev) == 0, f"{tag}: {len(ev)} voxels outside the footprint are NaN"
        for p in (p_inf, p_nan):
            mine = ev[ev[:, 0] == p[0]]
            dd, dh, dw = _reach(c, mine, p)
            assert len(mine) == 0 or (int(dd.max()) <= max(1, halo) and int(dh.max()) <= 1 and int(dw.max()) <= 1), \
                f"{tag}: NaN up to ({int(dd.max())}, {int(dh.max())}, {int(dw.max())}) from the voxel {p}"
        assert int(extra.sum()) <= int(nf.sum()) * c.c_out
        clean = ~(nf | extra.any(-1))
        compare32(tag, c.kernel, dt, got, r.y, r.U, r.K, mask=clean.unsqueeze(-1).expand_as(got))
        want = _check_16bit(tag, run, got, compare=same_stored)
    assert torch.equal(torch.isnan(want), torch.isnan(got)) and (run.dtype == torch.bfloat16 or not bool(torch.isinf(want).any()))


@pytest.mark.parametrize("c", R.EDGE_CASES, ids=lambda c: c.name)
def test_fp16_stores_saturate(env, c):
    """|v| far above 65504 (a scale of 2e5 on a unit-variance sum, no activation; tests/test_conv3d_ref_cpu.py holds the reference to
    more than 20 % above +65504 and more than 20 % below -65504): the fp32 output is within the bound, the fp16 stores of both
    instances hold +-65504, never inf, and equal round16 of the fp32 output bit for bit."""
    L, ops = env
    base, tag = _edge_launch(env, c, "fp16", epilogue="none")
    run = base.variant(epi=0, scale=torch.full((c.c_out,), 2.0e5))
    r = run.ref(True)
    assert float((r.y > R.F16_MAX).double().mean()) > 0.2 and float((r.y < -R.F16_MAX).double().mean()) > 0.2
    with L.tuning(**run.knobs):
        a_s = run.run(F32, SLICE8, skip=True).cpu()[..., 8:8 + c.c_out]
        compare32(f"{tag} saturation", c.kernel, "fp16", a_s, r.y, r.U, r.K, abs_bar=False)
        want = _check_16bit(f"{tag} saturation", run, a_s)
    assert float(want.max()) == R.F16_MAX and float(want.min()) == -R.F16_MAX and not bool(torch.isinf(want).any())


# ---- the fused kernels: bit identity to their two-launch paths (which the tests above hold to float64) on hard operands ----------
def _fused_layers(env, dtype, specs, seed):
    """Layers [(c_in, c_out, kind, transposed, epi, with_floor)] with BatchNorm scales in +-(0.5 .. 1.5) and cycled floors."""
    L, ops = env
    g = torch.Generator().manual_seed(seed)
    out = []
    for ci, co, kind, tr, epi, with_floor in specs:
        w = (torch.randn((ci, co, 3, 3, 3) if tr else (co, ci, 3, 3, 3), generator=g) / (27 * ci / (8 if kind == L.CONV_T2 else 1)) ** 0.5).to(dtype).float()
        sign = torch.where(torch.rand(co, generator=g) < 0.5, -1.0, 1.0)
        bn = ((torch.rand(co, generator=g) + 0.5) * sign, torch.randn(co, generator=g) * 0.1, torch.randn(co, generator=g) * 0.1, torch.rand(co, generator=g) + 0.5)
        layer = ops.Conv3dLayer.build(w, kind=kind, transposed=tr, device="cuda", bn=bn, relu=bool(epi & L.EPI_RELU_PRE), relu_post=bool(epi & L.EPI_RELU_POST),
                                      floor=R.cycled_floor(co) if with_floor else None, dtype=dtype)
        out.append(layer)
    return out, g


@pytest.mark.parametrize("dt", list(R.DTYPES))
def test_tail_sweep_equals_the_two_layers_on_hard_operands(env, dt):
    """pscv_tail_sweep with tail_nbk = 1 (14 output planes: chunks of 6, 6 and 2) on a ragged 7 x 5 x 15 input against T2P8 followed by
    the 1-channel head's sweep: negative scales in both layers, cycled finite floors, -inf / +inf / NaN skip voxels: same logits."""
    L, ops = env
    dtype = R.DTYPES[dt]
    (up, head), g = _fused_layers(env, dtype, [(16, 8, L.CONV_T2, True, L.EPI_RELU_PRE, True), (8, 1, L.CONV_S1, False, 0, False)], 71)
    assert up.kind == L.CONV_T2P8 and head.kind == L.CONV_S1C1
    B, Di, Hi, Wi = 2, 7, 5, 15
    x = torch.randn(B, Di, Hi, Wi, 16, generator=g).to(dtype).cuda()
    skip = torch.randn(B, 2 * Di, 2 * Hi, 2 * Wi, 8, generator=g).to(dtype)
    for with_nonfinite in (False, True):
        if with_nonfinite:
            skip[0, 3, 2, 4], skip[1, 9, 7, 20], skip[1, 2, 9, 29] = -INF, INF, NAN
        sk = skip.cuda()
        with L.tuning(c1_sweep=2):
            two = ops.conv3d(ops.conv3d(x, up, skip=sk), head, out_dtype=F32).view(B, 2 * Di, 2 * Hi, 2 * Wi)
        with L.tuning(tail_nbk=1):
            got = ops.tail_sweep(x, up, head, skip=sk)
        torch.cuda.synchronize()
        assert got is not None and same_stored(got.cpu(), two.cpu()), f"tail sweep {dt} non-finite={with_nonfinite}"
        assert bool(torch.isnan(two).any()) == with_nonfinite and bool(torch.isfinite(two).any())


@pytest.mark.parametrize("dt", list(R.DTYPES))
def test_residual_block_equals_the_two_launches_on_hard_operands(env, dt):
    """pscv_conv3d_block8 with many depth chunks (block8_slots = 4096) on a ragged 13 x 9 x 15 volume against the two 8 -> 8 launches:
    negative scales, cycled finite floors in the first layer: same bits.  With -inf / +inf / NaN in the input (which is the residual
    too) the bits are the same outside the voxels' neighbourhood; inside it the two paths pair the planes of the intermediate volume
    differently (the block's pairs start at odd planes), so their zero-weight rows turn different halo voxels into NaN: there the test
    holds that the elements which are finite in both paths have the same bits."""
    L, ops = env
    dtype = R.DTYPES[dt]
    (l1, l2), g = _fused_layers(env, dtype, [(8, 8, L.CONV_S1P8, False, L.EPI_RELU_PRE, True), (8, 8, L.CONV_S1P8, False, L.EPI_RELU_POST, False)], 72)
    B, D, H, W = 2, 13, 9, 15
    x = torch.randn(B, D, H, W, 8, generator=g).to(dtype)
    near = torch.zeros(B, D, H, W, dtype=torch.bool)
    for with_nonfinite in (False, True):
        if with_nonfinite:
            for (b, d, h, w, ch), val in (((0, 3, 2, 4, 0), -INF), ((1, 9, 6, 11, 5), INF), ((1, 2, 7, 2, 7), NAN)):
                x[b, d, h, w, ch] = val
                near[b, max(d - 6, 0):d + 7, max(h - 2, 0):h + 3, max(w - 2, 0):w + 3] = True
        xc = x.cuda()
        want = ops.conv3d(ops.conv3d(xc, l1), l2, skip=xc).cpu()
        with L.tuning(block8_slots=4096):
            got = ops.conv3d_block8(xc, l1, l2, residual=True)
        torch.cuda.synchronize()
        assert got is not None
        got = got.cpu()
        assert same_bits(got[~near], want[~near]), f"block8 {dt} non-finite={with_nonfinite}"
        assert bool(torch.isfinite(want[~near]).all())
        both = torch.isfinite(got) & torch.isfinite(want)
        assert torch.equal(_bits(got)[both], _bits(want)[both])


@pytest.mark.parametrize("dt", list(R.DTYPES))
def test_prob_softargmin_logits_equal_conv3d_on_hard_operands(env, dt):
    """pscv_prob_softargmin's logits on a ragged 19 x 5 x 33 volume (chunks of 6, 6, 6 and 1 planes) against pscv_conv3d with the
    sweep variant of the head: a negative scale, RELU_PRE with a floor of -0.5: same bits."""
    L, ops = env
    dtype = R.DTYPES[dt]
    (head,), g = _fused_layers(env, dtype, [(8, 1, L.CONV_S1, False, L.EPI_RELU_PRE, False)], 73)
    assert head.kind == L.CONV_S1C1
    head = dataclasses.replace(head, scale=-head.scale.abs(), floor=torch.tensor([-0.5], device="cuda"))
    B, D, H, W = 2, 19, 5, 33
    x = torch.randn(B, D, H, W, 8, generator=g).to(dtype).cuda()
    dv = torch.stack([torch.linspace(2.0, 6.0, D), torch.linspace(1.0, 9.0, D)]).cuda().contiguous()
    with L.tuning(c1_sweep=2):
        fused = ops.prob_softargmin(x, head, dv)
        logits = ops.conv3d(x, head, out_dtype=F32).view(B, D, H, W)
    torch.cuda.synchronize()
    assert fused is not None and same_bits(fused["logits"].cpu(), logits.cpu())
    lg = logits.cpu()
    assert float((lg == -0.5).double().mean()) > 0.1 and float((lg > -0.5).double().mean()) > 0.1
