"""pscv_conv2d_ex (ops.conv2d) held to the float64 reference of tests/_conv2d_ref.py: every PSCV_C2 instantiation of the streaming
kernel and every instantiation of the persistent weights-in-LDS kernel, in fp16 and bf16, at the smallest sizes at which each path
can go wrong (the case table lives in _conv2d_ref.py; tests/test_conv2d_ref_cpu.py checks it against the dispatch table and checks
the operands without a GPU).

What is asserted:
  * fp32 outputs, per element: |got - ref| <= c 2^-24 U with U = |scale| (|w| conv |x|) + |bias| + |skip| (``BOUND``: 4 x the worst
    ratio measured over all cases of a kernel and storage type on an MI355X, rounded up to one digit; DESIGN.md section 5 holds the
    table), never above K + 3 (the worst case of an fp32 sum of K exact products in any order plus the epilogue's three roundings,
    _conv2d_ref.py) and never looser than the 3e-5 max |ref| + 1e-6 of tests/test_gpu_conv2d.py;
  * 16-bit outputs equal ``round16`` of the fp32 output of the same operands bit for bit, on the staged epilogue (16-byte stores
    through an LDS row: slice offsets and strides multiples of 8) and on the direct one (an offset of 4, c_out off the tile);
  * every output map starts as NaN: a pixel, parity or blockIdx.y half that is not written, or written twice into another's place,
    shows as a NaN or a wrong value; the channels beside a written slice keep their NaN bits, the NaN beside a skip slice stays out;
  * non-finite values behave as in torch (see test_non_finite_values_behave_like_torch).

The input map has no channel stride in the ABI (it is always dense), so only the skip and the output are slices of wider tensors.
Out of scope, like the zero-weight rows of the conv3d depth sweeps (tests/test_gpu_conv3d.py): an ``inf`` ACTIVATION multiplied by the
zero weights of the k padding (k k c_in_padded is no multiple of 32) or of padded input channels may give NaN where ATen gives inf."""
import json
import os

import pytest
import torch

import _conv2d_ref as R

pytestmark = pytest.mark.gpu

# (kernel, storage type): bound c in units of 2^-24 U.    worst measured ratio (MI355X)    4 x worst
BOUND = {
    ("stream", "fp16"): 20,                              # 2.656 (3 -> 64 k3 s1, 3 x 13 x 47)  10.6
    ("stream", "bf16"): 9,                               # 2.237                              8.9
    ("wlds", "fp16"): 8,                                 # 1.921                              7.7
    ("wlds", "bf16"): 7,                                 # 1.602                              6.4
}
WORST = {}
NAN = float("nan")


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from wild_deep_mvs_amd import _lib as L, ops
    L.lib()
    yield L, ops
    print("\n[parity] conv2d ref: worst |got - ref| / (2^-24 U) per kernel and storage type", flush=True)
    for (kern, dt), v in sorted(WORST.items()):
        print(f"[parity] conv2d ref worst {kern:7s} {dt:5s} {v:.3f} (bound {BOUND[(kern, dt)]})", flush=True)
    path = os.environ.get("PSCV_CONV2D_ERR_TABLE")
    if path:
        with open(path, "w") as fh:
            json.dump({f"{kern}/{dt}": v for (kern, dt), v in sorted(WORST.items())}, fh, indent=1)


def _layer(ops, c, o, dtype):
    return ops.Conv2dLayer.build(o["w"], stride=c.stride, device="cuda", bn=o["bn"], conv_bias=o["conv_bias"], relu=o["neg_slope"] == 0.0,
                                 leaky=0.1 if o["neg_slope"] == 0.1 else None, dtype=dtype)


def _check_fold(layer, o):
    """The layer's folded epilogue vectors (Conv2dLayer.build on the device) become the reference's operands.  They are the CPU fold
    (_conv2d_ref.fold_bn, pinned by the CPU file) up to the device's fp32 sqrt and division, which are within 2 ulp of the correctly
    rounded ones: 1e-6 relative on the scale, 1e-6 of the O(1) terms beta and mean * scale on the bias."""
    for got, want in ((layer.scale, o["scale"]), (layer.bias, o["bias"])):
        assert (got is None) == (want is None)
        if got is not None:
            torch.testing.assert_close(got.cpu(), want, rtol=1e-6, atol=1e-6)
    o["scale"] = None if layer.scale is None else layer.scale.cpu()
    o["bias"] = None if layer.bias is None else layer.bias.cpu()


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def compare32(tag, kern, dt, got, ref_y, U, K):
    """fp32 ``got`` against the float64 ``ref_y``: NaN and inf exactly where the reference has them, the rest within the bound."""
    got = got.detach().double().cpu()
    assert got.shape == ref_y.shape, (tag, got.shape, ref_y.shape)
    nan = torch.isnan(ref_y)
    assert torch.equal(torch.isnan(got), nan), f"{tag}: NaN at {int(torch.isnan(got).sum())} elements, reference at {int(nan.sum())}"
    inf = torch.isinf(ref_y)
    assert torch.equal(got[inf], ref_y[inf]), f"{tag}: inf elements differ"
    fin = ~(nan | inf)
    err = (got - ref_y).abs()[fin]
    ratio = float((err / (2.0 ** -24 * U[fin])).max())
    ref_max = float(ref_y[fin].abs().max())
    WORST[(kern, dt)] = max(WORST.get((kern, dt), 0.0), ratio)
    bound = min(BOUND[(kern, dt)], K + 3)
    line = f"[parity] conv2d ref {tag}: max err / (2^-24 U) = {ratio:.3f} (bound {bound}, K + 3 = {K + 3}) max_abs={float(err.max()):.3e} (ref max {ref_max:.3e})"
    print(line, flush=True)
    assert ratio <= bound, line
    assert float(err.max()) <= 3e-5 * ref_max + 1e-6, line


def _wide(t, width, off, fill=NAN):
    """``t`` [..., c] as channels [off, off + c) of a new [..., width] tensor whose other channels hold ``fill``."""
    out = torch.full(t.shape[:-1] + (width,), fill, dtype=t.dtype)
    out[..., off:off + t.shape[-1]] = t
    return out


class Launches:
    """The launches of one (case, size) and their references; ``parities`` = (-1,) or (0, 1, 2, 3) into one map."""

    def __init__(self, ops, c, dtype, B, Hi, Wi, epilogue):
        self.ops, self.c, self.dtype = ops, c, dtype
        self.parities = (0, 1, 2, 3) if c.parity else (-1,)
        self.ops_ = [R.make_operands(c, dtype, B, Hi, Wi, epilogue=epilogue, parity=p) for p in self.parities]
        self.layers = [_layer(ops, c, o, dtype) for o in self.ops_]
        for l, o in zip(self.layers, self.ops_):
            _check_fold(l, o)
        self.skip = self.ops_[0]["skip"]                 # [B,Hf,Wf,c_out]: one full-map skip for all parities
        self.full = tuple(self.skip.shape[:3])
        self.x = [o["x"].cuda() for o in self.ops_]

    def ref(self, with_skip):
        """(y, U) float64 [B,Hf,Wf,c_out], K."""
        c = self.c
        y = torch.full(self.full + (c.c_out,), NAN, dtype=torch.float64)
        U = y.clone()
        for p, o in zip(self.parities, self.ops_):
            sk = None
            if with_skip:
                sk = self.skip if p < 0 else self.skip[:, p >> 1::2, p & 1::2]
            r = R.conv2d(o["x"], o["w"], k=c.k, stride=c.stride, scale=o["scale"], bias=o["bias"], skip=sk, neg_slope=o["neg_slope"])
            y, U = R.place(r.y, y, 0, p), R.place(r.U, U, 0, p)
        return y, U, r.K

    def run(self, out_dtype, *, skip_off=None, skip_width=None, out_off=0, out_width=None):
        """All parities into one NaN-filled [B,Hf,Wf,out_width] map; the skip as channels [skip_off, ..) of a NaN-filled wide map."""
        c = self.c
        out = torch.full(self.full + (out_width or c.c_out,), NAN, dtype=out_dtype, device="cuda")
        skip = None if skip_off is None else _wide(self.skip, skip_width, skip_off).cuda()
        for p, x, layer in zip(self.parities, self.x, self.layers):
            self.ops.conv2d(x, layer, skip=skip, skip_coff=skip_off or 0, out=out, out_coff=out_off, parity=p)
        return out


def check_forms(tag, kern, dt, run, c_out, dtype):
    """The output forms of one (case, size): fp32 dense without and with a skip against float64, then the 16-bit forms against
    round16 of the fp32 output: dense, staged epilogue (offsets 8), direct epilogue (output offset 4, skip offset 4)."""
    y, U, K = run.ref(False)
    a = run.run(torch.float32)
    compare32(f"{tag} fp32", kern, dt, a, y, U, K)
    ys, Us, _ = run.ref(True)
    a_s = run.run(torch.float32, skip_off=8, skip_width=c_out + 16)
    compare32(f"{tag} fp32+skip", kern, dt, a_s, ys, Us, K)
    assert same_bits(run.run(dtype), R.round16(a, dtype)), f"{tag}: dense 16-bit output is not the rounded fp32 output"
    want = R.round16(a_s.cpu(), dtype)
    b = run.run(dtype, skip_off=8, skip_width=c_out + 16, out_off=8, out_width=c_out + 24).cpu()
    assert same_bits(b, _wide(want, c_out + 24, 8)), f"{tag}: staged 16-bit slice"
    c1 = run.run(dtype, skip_off=8, skip_width=c_out + 16, out_off=4, out_width=c_out + 8).cpu()
    assert same_bits(c1, _wide(want, c_out + 8, 4)), f"{tag}: direct 16-bit slice (out_coff = 4)"
    c2 = run.run(dtype, skip_off=4, skip_width=c_out + 8, out_off=8, out_width=c_out + 24).cpu()
    assert same_bits(c2, _wide(want, c_out + 24, 8)), f"{tag}: direct 16-bit slice (skip_coff = 4)"
    return a, a_s


@pytest.mark.parametrize("dt", list(R.DTYPES))
@pytest.mark.parametrize("c", R.STREAM_CASES, ids=lambda c: c.name)
def test_streaming_kernel_equals_float64_reference(env, c, dt):
    """Every PSCV_C2 instantiation at the sizes of its stride (one-pixel maps, ragged tiles on both axes, outputs 33 and 34 wide
    behind the parity-split staging, B = 2 and 3), the four parities of the k2 / k3 parity layers into one map, the 128-channel
    layers' two blockIdx.y halves, c_out = 20 and 8 (no full channel tile: the direct epilogue's channel guard)."""
    L, ops = env
    dtype = R.DTYPES[dt]
    ci = R.CASES.index(c)
    with L.tuning(conv2d_wlds=0):
        for si, (Hi, Wi) in enumerate(c.sizes):
            B = R.batch_of(si)
            run = Launches(ops, c, dtype, B, Hi, Wi, R.epilogue_of(ci, si))
            check_forms(f"{c.name} {dt} {B}x{Hi}x{Wi}", "stream", dt, run, c.c_out, dtype)


@pytest.mark.parametrize("dt", list(R.DTYPES))
@pytest.mark.parametrize("c", R.WLDS_CASES, ids=lambda c: c.name)
def test_weights_in_lds_kernel_ragged_map(env, c, dt):
    """conv2d_wlds = 2 on the ragged 2 x 45 x 70 map (36 tiles, one per workgroup): against float64 and bit for bit the streaming
    kernel, every output form."""
    L, ops = env
    dtype = R.DTYPES[dt]
    B, Hi, Wi = R.WLDS_RAGGED
    run = Launches(ops, c, dtype, B, Hi, Wi, R.epilogue_of(R.CASES.index(c), 0))
    res = {}
    for wl in (2, 0):
        with L.tuning(conv2d_wlds=wl):
            kern = "wlds" if wl else "stream"
            res[wl] = check_forms(f"{c.name} {dt} {B}x{Hi}x{Wi} wlds={wl}", kern, dt, run, c.c_out, dtype)
    for a, b in zip(res[0], res[2]):
        assert same_bits(a, b)


@pytest.mark.parametrize("dt", list(R.DTYPES))
@pytest.mark.parametrize("c", R.WLDS_CASES, ids=lambda c: c.name)
def test_weights_in_lds_kernel_loops_over_tiles(env, c, dt):
    """A tall 1 x Hi x 97 map with more than twice as many tiles as persistent workgroups (_conv2d_ref.tall_rows): every workgroup
    holds the next tile's brick in registers across a contraction, passes the barrier that frees the brick and reuses its staging
    row.  The whole output equals the streaming kernel's bit for bit in three forms (fp32, 16-bit staged, 16-bit direct, all with a
    skip) and the default knob's (>= 512 tiles: the same kernel); three 24-row bands are held to float64."""
    L, ops = env
    dtype = R.DTYPES[dt]
    Hi = R.tall_rows(c, torch.cuda.get_device_properties(0).multi_processor_count)
    Wi = R.TALL_W
    assert 4 * ((Hi + 7) // 8) >= 512
    run = Launches(ops, c, dtype, 1, Hi, Wi, R.epilogue_of(R.CASES.index(c), 1))
    co = c.c_out
    res = {}
    for wl in (2, 0, 1):
        with L.tuning(conv2d_wlds=wl):
            res[wl] = (run.run(torch.float32, skip_off=8, skip_width=co + 16),
                       run.run(dtype, skip_off=8, skip_width=co + 16, out_off=8, out_width=co + 24),
                       run.run(dtype, skip_off=4, skip_width=co + 8, out_off=4, out_width=co + 8))
    for wl in (0, 1):
        for name, a, b in zip(("fp32", "staged", "direct"), res[wl], res[2]):
            assert same_bits(a, b), f"{c.name} {dt}: {name} output of conv2d_wlds = 2 differs from conv2d_wlds = {wl}"
    f32, staged, direct = (t.cpu() for t in res[2])
    want = R.round16(f32, dtype)
    assert same_bits(staged, _wide(want, co + 24, 8)) and same_bits(direct, _wide(want, co + 8, 4))
    o = run.ops_[0]
    for r0 in (0, (Hi // 2) // 8 * 8 - 3, Hi - 24):
        lo, hi = max(r0 - 1, 0), min(r0 + 25, Hi)
        r = R.conv2d(o["x"][:, lo:hi], o["w"], k=3, stride=1, scale=o["scale"], bias=o["bias"], skip=run.skip[:, lo:hi], neg_slope=o["neg_slope"])
        rows = slice(r0 - lo, r0 - lo + 24)
        compare32(f"{c.name} {dt} 1x{Hi}x{Wi} rows {r0}..{r0 + 23}", "wlds", dt, f32[:, r0:r0 + 24], r.y[:, rows], r.U[:, rows], r.K)


NONFINITE = [c for c in R.CASES if c.name in ("32to32k3s1", "16to16k3s1", "8to16k5s2", "wlds32to32")]


@pytest.mark.parametrize("dt", list(R.DTYPES))
@pytest.mark.parametrize("slope", [0.0, 0.1], ids=["relu", "leaky"])
@pytest.mark.parametrize("c", NONFINITE, ids=lambda c: c.name)
def test_non_finite_values_behave_like_torch(env, c, slope, dt):
    """Per kernel and epilogue form (fp32, staged, direct): a NaN activation gives NaN exactly on ATen's footprint (the padded k
    steps of 16 -> 16 k3 and 8 -> 16 k5 read a pixel of the same footprint with zero weights: no spill); a NaN skip element gives a
    NaN output element; -inf as a skip element gives 0 under ReLU and -inf under LeakyReLU; +inf stays +inf in fp32 and bf16 and is
    stored as 65504 in fp16 (-inf under LeakyReLU as -65504)."""
    L, ops = env
    dtype = R.DTYPES[dt]
    kern = c.kernel
    B, (Hi, Wi) = 2, ((9, 33) if c.stride == 1 else (9, 67))
    run = Launches(ops, c, dtype, B, Hi, Wi, "bn_relu" if slope == 0.0 else "bias_leaky")
    o = run.ops_[0]
    x = o["x"].clone()
    x[0, Hi // 2, Wi // 2, 1] = NAN
    x[1, 0, 0, c.c_in - 1] = NAN
    o["x"], run.x = x, [x.cuda()]
    _, Ho, Wo = run.full
    sk = run.skip
    p_nan, p_ninf, p_ninf2, p_pinf = (0, Ho - 1, Wo - 2, 3), (1, Ho - 1, Wo - 1, 0), (0, 0, Wo // 2 + 5, 9), (1, Ho // 2, Wo - 1, 13)
    sk[p_nan], sk[p_ninf], sk[p_ninf2], sk[p_pinf] = NAN, -float("inf"), -float("inf"), float("inf")
    ys, Us, K = run.ref(True)
    n_nan = int(torch.isnan(ys).sum())
    assert c.c_out * 8 < n_nan < ys.numel() // 4 and bool(torch.isnan(ys[p_nan]))
    assert float(ys[p_pinf]) == float("inf") and float(ys[p_ninf]) == float(ys[p_ninf2]) == (0.0 if slope == 0.0 else -float("inf"))
    co = c.c_out
    with L.tuning(conv2d_wlds=2 if kern == "wlds" else 0):
        a = run.run(torch.float32, skip_off=8, skip_width=co + 16)
        staged = run.run(dtype, skip_off=8, skip_width=co + 16, out_off=8, out_width=co + 24).cpu()
        direct = run.run(dtype, skip_off=8, skip_width=co + 16, out_off=4, out_width=co + 8).cpu()
    compare32(f"{c.name} {dt} non-finite slope {slope}", kern, dt, a, ys, Us, K)
    want = R.round16(a.cpu(), dtype)
    big = R.F16_MAX if dtype == torch.float16 else float("inf")
    assert float(want[p_pinf]) == big and float(want[p_ninf]) == (0.0 if slope == 0.0 else -big)
    for name, got, off in (("staged", staged, 8), ("direct", direct, 4)):
        inner = got[..., off:off + co]
        nan = torch.isnan(want)
        assert torch.equal(torch.isnan(inner), nan), f"{name}: NaN footprint"
        assert torch.equal(inner[~nan], want[~nan]), f"{name}: values beside the NaN footprint"
        assert not bool(torch.isinf(inner).any()) or dtype == torch.bfloat16
        outer = torch.cat([got[..., :off], got[..., off + co:]], -1)
        assert same_bits(outer, torch.full_like(outer, NAN))


@pytest.mark.parametrize("c", [c for c in R.CASES if c.name in ("16to16k3s1", "wlds32to32")], ids=lambda c: c.name)
def test_fp16_stores_saturate(env, c):
    """|v| far above 65504 (a scale of 2e5 on a unit-variance sum, no activation): the fp16 stores of both epilogue forms hold
    +-65504, never inf, and still equal round16 of the fp32 output."""
    L, ops = env
    dtype = torch.float16
    run = Launches(ops, c, dtype, 2, 9, 33, "none")
    scale = torch.full((c.c_out,), 2.0e5)
    run.layers[0].scale, run.ops_[0]["scale"] = scale.cuda(), scale
    co = c.c_out
    with L.tuning(conv2d_wlds=2 if c.kernel == "wlds" else 0):
        a = run.run(torch.float32, skip_off=8, skip_width=co + 16)
        staged = run.run(dtype, skip_off=8, skip_width=co + 16, out_off=8, out_width=co + 24).cpu()
        direct = run.run(dtype, skip_off=8, skip_width=co + 16, out_off=4, out_width=co + 8).cpu()
    ys, Us, K = run.ref(True)
    compare32(f"{c.name} fp16 saturation", c.kernel, "fp16", a, ys, Us, K)
    assert float((ys > R.F16_MAX).double().mean()) > 0.2 and float((ys < -R.F16_MAX).double().mean()) > 0.2
    want = R.round16(a.cpu(), dtype)
    assert float(want.max()) == R.F16_MAX and float(want.min()) == -R.F16_MAX and not bool(torch.isinf(want).any())
    assert same_bits(staged, _wide(want, co + 24, 8)) and same_bits(direct, _wide(want, co + 8, 4))
