"""No GPU: the float64 reference of tests/_conv3d_ref.py pinned to float64 ATen, its error unit and its epilogue truth table, the
store model ``round16``, the case table that tests/test_gpu_conv3d_ref.py runs checked against the dispatch code of csrc/conv3d*.hip
and the knob table, an fp32 model of the kernels' chains held to the (K + 3) 2^-24 U bound on every row's operands, and the
conditions that the GPU file's saturation and non-finite operand sets rely on."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _conv3d_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "wild_deep_mvs_amd", "csrc")
INF, NAN = float("inf"), float("nan")


def _ncdhw(t):
    return t.permute(0, 4, 1, 2, 3)


def _aten(x, w, kind, transposed):
    xn = _ncdhw(x.double())
    if kind == "T2":
        y = F.conv_transpose3d(xn, w.double(), stride=2, padding=1, output_padding=1)
    elif transposed:
        y = F.conv_transpose3d(xn, w.double(), stride=1, padding=1)
    else:
        y = F.conv3d(xn, w.double(), stride=1 if kind == "S1" else 2, padding=1)
    return y.permute(0, 2, 3, 4, 1)


KINDS = [("S1", False), ("S1", True), ("S2", False), ("T2", True)]
SHAPES = [(2, 1, 1, 1, 8, 4), (1, 2, 2, 2, 8, 12), (2, 1, 5, 3, 16, 8), (3, 5, 1, 4, 8, 1), (1, 3, 4, 1, 8, 16), (2, 5, 7, 9, 16, 8), (1, 6, 3, 11, 8, 20)]


@pytest.mark.parametrize("kind,transposed", KINDS)
def test_reference_equals_float64_aten(kind, transposed):
    """Odd sizes, 1 x 1 x 1, a size-1 axis in each position, B = 1..3; the error unit is the same expression on absolute values."""
    g = torch.Generator().manual_seed(len(kind) + 7 * transposed)
    for B, D, H, W, ci, co in SHAPES:
        x = torch.randn(B, D, H, W, ci + 8, generator=g).to(torch.float16)          # (channels past c_in hold values: they must not be read)
        w = torch.randn((ci, co, 3, 3, 3) if transposed else (co, ci, 3, 3, 3), generator=g).to(torch.float16).float()
        r = R.conv3d(x, w, kind=kind, transposed=transposed, K=5)
        want = _aten(x[..., :ci], w, kind, transposed)
        assert r.y.shape == want.shape == (B,) + R.out_dhw(kind, D, H, W) + (co,) and r.K == 5 and torch.equal(r.y, r.v)
        wantU = _aten(x[..., :ci].abs(), w.abs(), kind, transposed)
        torch.testing.assert_close(r.y, want, rtol=0, atol=1e-12 * float(wantU.max()))
        assert bool(((r.y - want).abs() <= 1e-12 * wantU + 1e-300).all())
        torch.testing.assert_close(r.U, wantU, rtol=0, atol=1e-12 * float(wantU.max()))
        assert bool((r.U >= r.v.abs() * (1 - 1e-12)).all())
    assert R.out_dhw("S2", 5, 5, 33) == (3, 3, 17) and R.out_dhw("T2", 3, 5, 17) == (6, 10, 34)
    with pytest.raises(ValueError):
        R.out_dhw("S3", 1, 1, 1)


@pytest.mark.parametrize("kind,transposed", KINDS)
def test_folded_epilogue_equals_aten_and_the_error_unit_bounds_it(kind, transposed):
    """scale / bias as Conv3dLayer.build folds BatchNorm3d, against F.batch_norm + F.relu in float64, in both orders of ReLU and skip;
    U >= |v| elementwise; U does not change under sign flips of x, w and the skip."""
    g = torch.Generator().manual_seed(3 + len(kind))
    B, D, H, W, ci, co = 2, 3, 5, 6, 8, 12
    x = torch.randn(B, D, H, W, ci, generator=g).to(torch.bfloat16)
    w = torch.randn((ci, co, 3, 3, 3) if transposed else (co, ci, 3, 3, 3), generator=g).to(torch.bfloat16).float()
    sign = torch.where(torch.rand(co, generator=g) < 0.5, -1.0, 1.0)
    bn = ((torch.rand(co, generator=g) + 0.5) * sign, torch.randn(co, generator=g), torch.randn(co, generator=g), torch.rand(co, generator=g) + 0.5)
    cb = torch.randn(co, generator=g)
    skip = torch.randn((B,) + R.out_dhw(kind, D, H, W) + (co + 8,), generator=g).to(torch.bfloat16)
    scale, bias = R.fold_bn(*bn, conv_bias=cb)
    conv = _ncdhw(_aten(x, w, kind, transposed)) + cb.double().view(1, -1, 1, 1, 1)
    normed = F.batch_norm(conv, bn[2].double(), bn[3].double(), bn[0].double(), bn[1].double(), False, 0.0, 1e-5)
    sk = _ncdhw(skip[..., 4:4 + co].double())
    for pre, post, want in ((True, False, F.relu(normed) + sk), (False, True, F.relu(normed + sk)), (True, True, F.relu(F.relu(normed) + sk)),
                            (False, False, normed + sk)):
        r = R.conv3d(x, w, kind=kind, transposed=transposed, scale=scale, bias=bias, skip=skip, skip_coff=4, relu_pre=pre, relu_post=post)
        assert bool(((_ncdhw(r.y) - want).abs() <= 4e-6 * _ncdhw(r.U)).all())          # (the fold is fp32: 2^-24 relative per vector)
        assert bool((r.U >= r.v.abs() * (1 - 1e-12)).all()) and bool((r.U >= r.y.abs() * (1 - 1e-12)).all())
        assert float((r.y == 0).double().mean()) > 0.1 or not post
        for fx, fw, fs in ((-1, 1, 1), (1, -1, 1), (1, 1, -1), (-1, -1, -1)):
            r2 = R.conv3d((x.float() * fx).to(x.dtype), w * fw, kind=kind, transposed=transposed, scale=scale, bias=bias, skip=(skip.float() * fs).to(skip.dtype),
                          skip_coff=4, relu_pre=pre, relu_post=post)
            assert torch.equal(r2.U, r.U)
    assert float((scale < 0).double().mean()) > 0.2
    try:
        from wild_deep_mvs_amd import ops, _lib as L
        layer = ops.Conv3dLayer.build(w, kind={"S1": L.CONV_S1, "S2": L.CONV_S2, "T2": L.CONV_T2}[kind], transposed=transposed, device="cpu", bn=bn,
                                      conv_bias=cb, relu=True, dtype=torch.bfloat16)
    except Exception:                                          # no host library: the fold is still pinned by the lines above
        layer = None
    if layer is not None:
        assert torch.equal(layer.scale, scale) and torch.equal(layer.bias, bias) and layer.epi == L.EPI_RELU_PRE


def test_nan_and_inf_activations_have_atens_footprint():
    g = torch.Generator().manual_seed(5)
    for kind, transposed in KINDS:
        x = torch.randn(2, 5, 6, 7, 8, generator=g, dtype=torch.float64)
        x[0, 2, 3, 3, 1], x[1, 1, 2, 5, 7] = NAN, INF
        w = torch.randn((8, 4, 3, 3, 3) if transposed else (4, 8, 3, 3, 3), generator=g, dtype=torch.float64)
        w[1 if not transposed else slice(None), slice(None) if not transposed else 1] = 0          # 0 * NaN = NaN in ATen and in an MFMA
        got, want = R.conv3d(x, w, kind=kind, transposed=transposed).y, _aten(x, w, kind, transposed)
        assert torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(torch.isinf(got), torch.isinf(want))
        assert torch.equal(got[torch.isinf(got)], want[torch.isinf(want)])
        nf = R.acc_nonfinite(x, w, kind=kind, transposed=transposed)
        assert torch.equal(nf, (~torch.isfinite(want)).any(-1)) and 2 <= int(nf.sum()) <= 2 * 27


def test_epilogue_truth_table():
    """On scalars: the floor is ignored without RELU_PRE; a finite floor; a -inf floor; PRE + POST; a -inf skip with POST gives 0; NaN
    passes both clamps; +inf stays."""
    t = lambda *v: torch.tensor(v, dtype=torch.float64)
    acc = t(-2.0, -0.3, 0.1, 3.0, NAN, -INF, INF)
    n = acc.numel()

    def run(floor=None, skip=None, **kw):
        y, v = R.epilogue(acc.view(1, n).t().contiguous().view(n, 1), floor=None if floor is None else t(floor), skip=None if skip is None else t(*skip).view(n, 1), **kw)
        return y.view(-1), v.view(-1)

    def same(a, b):
        return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a[~torch.isnan(a)], b[~torch.isnan(b)])
    y, v = run()
    assert same(y, acc) and same(v, acc)
    assert same(run(floor=0.25)[0], acc) and same(run(floor=0.25, relu_post=True)[0], t(0, 0, 0.1, 3, NAN, 0, INF))          # floor ignored without RELU_PRE
    assert same(run(relu_pre=True)[0], t(0, 0, 0.1, 3, NAN, 0, INF))                                                  # relu(-inf) = 0, NaN stays
    assert same(run(relu_pre=True, floor=0.25)[0], t(0.25, 0.25, 0.25, 3, NAN, 0.25, INF))
    assert same(run(relu_pre=True, floor=-0.5)[0], t(-0.5, -0.3, 0.1, 3, NAN, -0.5, INF))
    assert same(run(relu_pre=True, floor=-INF)[0], acc)                                                               # a linear channel
    sk = (1.0, -1.0, -1.0, -INF, 0.0, INF, -INF)
    assert same(run(relu_pre=True, floor=-0.5, skip=sk)[0], t(0.5, -1.3, -0.9, -INF, NAN, INF, NAN))
    assert same(run(relu_pre=True, relu_post=True, floor=-0.5, skip=sk)[0], t(0.5, 0, 0, 0, NAN, INF, NAN))            # -inf skip, POST -> 0
    assert same(run(relu_post=True, skip=sk)[0], t(0, 0, 0, 0, NAN, NAN, NAN))
    assert same(run(relu_post=True, skip=(0.0,) * 7)[0], t(0, 0, 0.1, 3, NAN, 0, INF))
    # scale and bias come first, per channel
    y, _ = R.epilogue(t(1.0, 1.0).view(1, 2), scale=t(-2.0, 3.0), bias=t(0.5, -INF), floor=t(-1.0, 0.25), relu_pre=True)
    assert torch.equal(y.view(-1), t(-1.0, 0.25))
    assert R.cycled_floor(6).tolist() == [-0.5, 0.25, -INF, 0.0, -0.5, 0.25]


def test_round16_models_the_engines_stores():
    """pscv_common.h: f32_to_f16_bits / pack_f16x2 round to nearest even and saturate at +-65504, true inf included; bf16 as torch; NaN
    stays NaN in both."""
    f16, bf16 = torch.float16, torch.bfloat16
    v = torch.tensor([65504.0, 65519.9, 65520.0, 1e6, INF, -65519.9, -65520.0, -INF, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 2.0 ** -25, 2.0 ** -24 * 1.5, -0.0])
    want = torch.tensor([65504.0, 65504.0, 65504.0, 65504.0, 65504.0, -65504.0, -65504.0, -65504.0, 1.0, 1.0 + 2.0 ** -9, 0.0, 2.0 ** -23, -0.0])
    for src in (v, v.double()):
        got = R.round16(src, f16)
        assert got.dtype == f16 and torch.equal(got.double(), want.double()) and bool(torch.signbit(got[-1]))
    for dt in (f16, bf16):
        assert bool(torch.isnan(R.round16(torch.tensor([NAN]), dt))) and R.round16(torch.tensor([NAN]), dt).dtype == dt
    b = R.round16(torch.tensor([INF, -INF, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8]), bf16)
    assert torch.equal(b.double(), torch.tensor([INF, -INF, 1.0, 1.0 + 2.0 ** -6], dtype=torch.float64))


def _src(name):
    return open(os.path.join(CSRC, name)).read()


def test_case_table_covers_the_dispatch_code():
    """Every PSCV_CONV_CASE line of conv3d.hip has its rows (x S1 / S2 / T2, large and small tiles, every conv_small_nt that divides the
    tile count, the tall tile), every (c_in, c_out) the sweep / wide / c1 / t2p8 / cat2 / stride-2 launchers accept has a row, and every
    knob a row or a size names is in PSCV_KNOB_TABLE: a new dispatch line without a row, or a renamed knob, fails here."""
    conv = _src("conv3d.hip")
    lines = [(int(a), int(b)) for a, b in re.findall(r"PSCV_CONV_CASE\((\d+), (\d+)\)", conv)]
    assert len(lines) == len(set(lines)) == 9 and lines == R.BRICK_LINES
    brick = [c for c in R.CASES if c.kernel == "brick"]
    for ci, nt in lines:
        rows = [c for c in brick if (c.c_in, (c.c_out + 15) // 16) == (ci, nt)]
        splits = [n for n in (1, 2, 4) if n <= nt and nt % n == 0]
        for kind in ("S1", "T2"):
            have = [c.knobs for c in rows if c.kind == kind and c.transposed == (kind == "T2")]
            assert sum(k["conv_small_tiles"] == 0 and k["conv_tall64"] == 0 for k in have) == 1, (ci, nt, kind)
            assert sorted(k["conv_small_nt"] for k in have if k["conv_small_tiles"] == 1) == splits, (ci, nt, kind)
        s2 = sorted(c.knobs["conv_small_nt"] for c in rows if c.kind == "S2")
        assert s2 == ([0] if nt == 1 else splits), (ci, nt)
        assert any(c.knobs["conv_tall64"] == 2 for c in rows) == (ci == 64)
    assert {c.c_in for c in brick if c.transposed and c.kind == "S1"} == {8, 16, 32, 64}
    assert all(c.knobs["conv_wide"] == 0 and c.knobs["conv_s2_sweep"] == 0 for c in brick)          # neither takes a brick row away
    # the launchers' (c_in, c_out) conditions, as written in the sources
    m = re.search(r"\(\(c_in == 8 \|\| c_in == 16 \|\| c_in == 32\) && c_out == 8\) \|\| \(c_in == 16 && c_out == 16\)", conv)
    assert m, "pscv_conv3d: the S1P8 condition changed"
    sweeps = {(c.c_in, c.c_out) for c in R.CASES if c.kernel in ("pair", "kdm", "narrow") and not c.cat2}
    assert sweeps == {(8, 8), (16, 8), (32, 8), (16, 16)}
    assert re.search(r"return c_in == 32 \? conv3d_sweep8_launch\(c\) : conv3d_sweepc_launch\(c\);", conv)
    assert {c.c_in for c in R.CASES if c.kernel in ("pair", "kdm")} == {32} and {c.c_in for c in R.CASES if c.kernel == "narrow"} == {8, 16}
    assert re.search(r'PSCV_CHECK_ARG\(c_out == 8 \|\| c_out == 16, "pscv_conv3d_cat2', conv)
    assert sorted(c.c_out for c in R.CASES if c.cat2) == [8, 16] and all(c.c_in == 16 and c.kernel == "narrow" for c in R.CASES if c.cat2)
    assert re.search(r"PSCV_CHECK_ARG\(c_in == 16 && c_out == 8, \"pscv_conv3d: the parity-pair kernel", conv)
    assert [(c.c_in, c.c_out, c.kind) for c in R.CASES if c.kernel == "t2p8"] == [(16, 8, "T2")]
    assert re.search(r"PSCV_CHECK_ARG\(c_out == 1 && \(c_in == 8 \|\| c_in == 16\), \"pscv_conv3d: the 1-channel kernel", conv)
    c1 = _src("conv3d_c1.hip")
    assert re.search(r"if \(c\.c_in == 8 && g_c1_sweep &&", c1) and "constexpr int C1_NB_MAX = 2;" in c1
    assert {(c.c_in, c.knobs["c1_sweep"]) for c in R.CASES if c.kernel == "c1"} == {(8, 0), (16, 0), (16, 2)}
    assert [(c.c_in, c.knobs["c1_sweep"]) for c in R.CASES if c.kernel == "c1sweep"] == [(8, 2)]
    wide = _src("conv3d_wide.hip")
    assert re.search(r"if \(!\(\(c\.c_in == 32 \|\| c\.c_in == 64\) && \(c\.c_out == 32 \|\| c\.c_out == 64\)\)\) return 1;", wide)
    assert len(re.findall(r"widep_launch<H, (\d+), (\d+)>\(a, nblk, c\.st\)", wide)) == 4
    assert {(c.c_in, c.c_out) for c in R.WIDE_CASES} == {(64, 64), (64, 32), (32, 64), (32, 32)} and all(c.knobs == {"conv_wide": 2} for c in R.WIDE_CASES)
    s2 = _src("conv3d_sweep_s2.hip")
    assert re.search(r"if \(!g_conv_s2_sweep \|\| c\.c_in != 8 \|\| c\.c_out > 32 \|\| c\.c_out % 4\) return 1;", s2)
    assert re.search(r"return nt == 1 \? s2s_launch<H, 1>\(a, nblk, c\.st\) : s2s_launch<H, 2>\(a, nblk, c\.st\);", s2)
    assert sorted(c.c_out for c in R.CASES if c.kernel == "s2sweep") == [16, 24, 32]           # one tile, a ragged second tile, two tiles
    sw = _src("conv3d_sweep.hip")
    assert "const bool tall = !kdm && g_sweep_th16 && c.H >= 16;" in sw and "const int pd = g_sweep_kdm_pd > 0 ? g_sweep_kdm_pd : 1;" in sw
    assert {(c.knobs["sweep_kdm"], c.knobs["sweep_kdm_pd"]) for c in R.CASES if c.kernel == "kdm"} == {(1, 1), (1, 2), (2, 1), (2, 2)}
    assert {c.knobs["sweep_th16"] for c in R.CASES if c.kernel == "pair"} == {0, 1}
    for ci, co in ((8, 8), (16, 8), (16, 16)):
        assert {c.knobs["sweepc_pd"] for c in R.CASES if c.kernel == "narrow" and (c.c_in, c.c_out) == (ci, co)} >= {1, 2, 3}
    # knob names
    knobs = set(re.findall(r'X\("(\w+)", g_\w+, -?\d+\)', _src("pscv_common.h")))
    assert len(knobs) >= 27
    used = set()
    for c in R.CASES:
        used |= set(c.knobs) | set(c.twin or {})
        for si, (D, H, W, kn) in enumerate(c.sizes):
            used |= set(R.resolve_knobs(c, R.batch_of(si), D, H, W, kn))
    assert used <= knobs, f"rows name knobs that do not exist: {sorted(used - knobs)}"
    assert used >= {"sweep_dc", "s2s_slots", "c1_nb", "conv_small_nt", "conv_tall64", "conv_wide", "sweepc_pd", "sweep_kdm_pd", "sweep_th16", "c1_sweep", "conv_s2_sweep"}
    # what else the GPU file relies on
    assert len({c.name for c in R.CASES}) == len(R.CASES) and all(c.halo <= (6 if c.kernel in ("c1", "c1sweep") else 2) for c in R.CASES)
    assert {c.kernel for c in R.EDGE_CASES} == {c.kernel for c in R.CASES}
    assert {(c.kernel, c.kind) for c in R.EDGE_CASES if c.kernel == "brick"} == {("brick", "S1"), ("brick", "S2"), ("brick", "T2")}
    for c in R.CASES:
        assert c.sizes[0] == R.ONE and len(c.sizes) >= 2 and {R.batch_of(i) for i in range(len(c.sizes))} == {2, 3}
        assert c.transposed or c.kind != "T2"
    eps = [R.epilogue_of(R.CASES.index(c), si) for c in R.CASES for si in range(len(c.sizes))]
    assert all(abs(eps.count(e) / len(eps) - 0.25) < 0.05 for e in R.EPILOGUES)


def test_sizes_cut_the_tiles_and_the_depth_chunks_they_are_meant_to():
    """Per row: a size with two tiles per axis whose last tile is one voxel thick (tile constants restated from the kernels); for the
    sweeps a chunk in which the plane ring wraps at least twice and a forced seam whose last chunk holds a single plane; the brick
    variant of the 1-channel head never gets more than C1_NB_MAX blocks per workgroup (its staging registers and LDS are sized for 2)."""
    tile = {("brick", "S1", 0): (4, 4, 16), ("brick", "S1", 1): (1, 4, 16), ("brick", "S2", 0): (2, 2, 16), ("brick", "T2", 0): (2, 4, 16),
            ("brick", "T2", 1): (1, 4, 16), "wide": (4, 4, 16), "t2p8": (2, 4, 16)}
    ring = {"pair": 6, "narrow": 6, "kdm": 3, "s2sweep": 5, "c1sweep": 16}         # LDS plane slots; a slot is written once per input plane
    for c in R.CASES:
        seams = wraps = False
        for si, (D, H, W, kn) in enumerate(c.sizes):
            B = R.batch_of(si)
            knobs = R.resolve_knobs(c, B, D, H, W, kn)
            if c.kernel == "c1":
                assert knobs.get("c1_nb", 0) <= 2, c.name
            if si == 0:
                continue
            if c.kernel in ("brick", "wide", "t2p8"):
                t = tile.get(c.kernel) or tile[(c.kernel, c.kind, 0 if c.kind == "S2" else c.knobs["conv_small_tiles"])]
                if c.knobs.get("conv_tall64") == 2:
                    t = (4, 8, 16)
                dims = R.out_dhw("S2", D, H, W) if c.kind == "S2" else (D, H, W)
                assert all(n == tt + 1 for n, tt in zip(dims, t)), (c.name, dims, t)
                assert B * 8 < 1024                                            # (launch_kind: the small variants apply below 1024 large tiles)
            else:
                th = 16 if (c.kernel == "pair" and knobs.get("sweep_th16")) else 4 if c.kernel in ("c1", "c1sweep") else 8
                tw = 32 if c.kernel in ("c1", "c1sweep") else 16
                _, Ho, Wo = R.out_dhw(c.kind, D, H, W)
                assert Ho == th + 1 and Wo == tw + 1, (c.name, Ho, Wo)
                chunks = R.depth_chunks(c, B, D, H, W, knobs)
                assert sum(chunks) == R.out_dhw(c.kind, D, H, W)[0]
                seams |= len(chunks) >= 2 and chunks[-1] == 1
                if c.kernel in ring:      # input planes written during the longest chunk (two per output plane at stride 2)
                    wraps |= max(chunks) * (2 if c.kernel == "s2sweep" else 1) >= 2 * ring[c.kernel]
        if c.kernel in ring or c.kernel == "c1":
            assert seams, f"{c.name}: no size with a one-plane last chunk"
        if c.kernel in ring:
            assert wraps, f"{c.name}: no chunk long enough for the ring to wrap twice"
    B, D, H, W, grid, tiles = R.long_volume(256)
    assert (B, D, H, W, grid, tiles) == (1, 13, 173, 33, 256, 528) and tiles >= 2 * grid + 3 and tiles >= 512
    for n_cu in (64, 104, 304):
        B, D, H, W, grid, tiles = R.long_volume(n_cu)
        assert tiles >= max(2 * grid + 3, 512) and tiles == B * -(-D // 4) * -(-H // 4) * -(-W // 16) and H % 4 == 1


def _sample_chain(c, o, r, g, n=48):
    """max |chain - v| / (2^-24 U) over ``n`` sampled output elements: the exact products of the 16-bit operands (exact in fp32: at
    most 22 significant bits) summed in float32 in a shuffled order with K - terms zeros, then the epilogue in fp32 (one fma, the clamp,
    the skip add, the clamp)."""
    wg = R.gather_weight(o["w"], c.kind, c.transposed)
    x = o["x"].double()
    shape = r.v.shape
    idx = torch.randint(0, r.v.numel(), (n,), generator=g)
    co = idx % shape[-1]
    vox = idx // shape[-1]
    prods = []
    for (kd, kh, kw), xs in R.taps(x, c.kind):
        prods.append(xs.reshape(-1, xs.shape[-1])[vox] * wg[co, :, kd, kh, kw])
    p = torch.cat(prods, 1)
    p32 = p.float()
    assert torch.equal(p32.double(), p)                                      # exact products
    K = R.k_terms(c)
    assert p32.shape[1] <= K or c.kind == "T2"
    pad = max(K - p32.shape[1], 0)
    p32 = torch.cat([p32, torch.zeros(n, pad)], 1).numpy()
    perm = torch.randperm(p32.shape[1], generator=g).numpy()
    acc = np.cumsum(p32[:, perm], axis=1, dtype=np.float32)[:, -1]           # a sequential float32 sum
    f32 = np.float32
    sc = np.ones(n, f32) if o["scale"] is None else o["scale"].numpy()[co]
    bi = np.zeros(n, f32) if o["bias"] is None else o["bias"].numpy()[co]
    v = (acc.astype(np.float64) * sc.astype(np.float64) + bi.astype(np.float64)).astype(f32)      # fma: one rounding
    if o["relu_pre"]:
        v = np.where(v < 0, f32(0), v)
    sk = o["skip"].float().reshape(-1, shape[-1])[vox, co].numpy()
    v = (v + sk).astype(f32)
    if o["relu_post"]:
        v = np.where(v < 0, f32(0), v)
    U = r.U.reshape(-1)[idx].numpy()
    return float(np.max(np.abs(v.astype(np.float64) - r.y.reshape(-1)[idx].numpy()) / (2.0 ** -24 * U)))


@pytest.mark.parametrize("c", R.CASES, ids=lambda c: c.name)
def test_operands_of_every_case_meet_the_conditions_of_the_bounds(c):
    """On every (row, size, storage type): the operands hold storage-type values, U > 0 at every output element, no non-finite
    reference value, |v| far below 65504 (the ordinary cases do not saturate), about half of the BatchNorm scales negative over the
    table; and an fp32 chain in a shuffled order stays within (K + 3) 2^-24 U -- the bound holds for the reference alone."""
    ci = R.CASES.index(c)
    g = torch.Generator().manual_seed(ci)
    K = R.k_terms(c)
    assert 32 <= K <= 27 * 64 and K % 32 == 0
    for dt, dtype in R.DTYPES.items():
        for si, (D, H, W, _) in enumerate(c.sizes):
            B = R.batch_of(si)
            o = R.make_operands(c, dtype, B, D, H, W, epilogue=R.epilogue_of(ci, si))
            assert o["x"].dtype == dtype and tuple(o["x"].shape) == (B, D, H, W, c.c_in) and torch.equal(o["w"], o["w"].to(dtype).float())
            assert tuple(o["w"].shape[:2]) == ((c.c_in, c.c_out) if c.transposed else (c.c_out, c.c_in))
            for with_skip in (False, True):
                r = R.reference(c, o, with_skip=with_skip)
                assert r.K == K and bool(torch.isfinite(r.y).all()) and bool(torch.isfinite(r.U).all()), (c.name, dt, D, H, W)
                assert float(r.U.min()) > 0 and float(r.v.abs().max()) < 100 < R.F16_MAX, (c.name, dt, D, H, W)
            ratio = _sample_chain(c, o, r, g)
            assert ratio <= K + 3, (c.name, dt, (D, H, W), ratio)
    o = R.make_operands(c, torch.float16, 2, *c.sizes[1][:3], epilogue="bn_relu_skip")
    assert o["bn"][0].abs().min() >= 0.5 and o["bn"][0].abs().max() <= 1.5


def test_about_half_of_the_scales_are_negative():
    neg = tot = 0
    for ci, c in enumerate(R.CASES):
        o = R.make_operands(c, torch.float16, 1, 1, 1, 1, epilogue="bn_skip_relupost")
        neg, tot = neg + int((o["scale"] < 0).sum()), tot + c.c_out
    assert 0.4 < neg / tot < 0.6


@pytest.mark.parametrize("c", R.EDGE_CASES, ids=lambda c: c.name)
def test_edge_operand_sets_meet_their_conditions(c):
    """What tests/test_gpu_conv3d_ref.py states about its saturation and non-finite operand sets, on the reference alone: with a scale
    of 2e5 more than 20 % of the values lie above +65504 and more than 20 % below -65504; the +inf and the NaN input voxel are inside
    the volume, in different batch items, and give the reference inf, NaN and (under ReLU) zeros from -inf; the three non-finite skip
    voxels and the -inf bias channel give each class under both ReLU orders."""
    B, D, H, W, _ = R.edge_size(c)
    o = R.make_operands(c, torch.float16, B, D, H, W, epilogue="none")
    o["scale"] = torch.full((c.c_out,), 2.0e5)
    r = R.reference(c, o, with_skip=True)
    assert float((r.y > R.F16_MAX).double().mean()) > 0.2 and float((r.y < -R.F16_MAX).double().mean()) > 0.2
    want = R.round16(r.y, torch.float16)
    assert float(want.max()) == R.F16_MAX and float(want.min()) == -R.F16_MAX and not bool(torch.isinf(want).any())
    # non-finite through the contraction
    p_inf, p_nan = R.nonfinite_voxels(c, D, H, W)
    assert p_inf[0] != p_nan[0] and all(0 <= a < n for p in (p_inf, p_nan) for a, n in zip(p, (B, D, H, W)))
    if c.kernel in ("c1", "c1sweep"):
        assert p_inf[1] % 6 in (2, 3) and p_nan[1] % 6 in (2, 3)
    for relu in (False, True):
        o = R.make_operands(c, torch.float16, B, D, H, W, epilogue="bn_relu_skip")
        o["relu_pre"] = relu
        o["x"][p_inf][1 % c.c_in], o["x"][p_nan][c.c_in - 1] = INF, NAN
        r = R.reference(c, o, with_skip=True)
        nf = R.acc_nonfinite(o["x"], o["w"], kind=c.kind, transposed=c.transposed)
        assert torch.equal(nf, (~torch.isfinite(R.reference(c, o, with_skip=False, relu_pre=False).v)).any(-1))
        assert bool(torch.isnan(r.y[1]).any()) and not bool(torch.isnan(r.y[0]).any()) and bool(torch.isinf(r.y[0]).any())
        assert bool(torch.isfinite(r.y[~nf]).all()) and 2 <= int(nf.sum()) <= 2 * 27
        if relu:
            assert bool((torch.isfinite(r.y[0]) & nf[0].unsqueeze(-1)).any()) or c.c_out == 1          # relu(-inf) = floor 0, finite
    # non-finite beside the contraction
    for pre, post in ((True, False), (False, True), (True, True)):
        o = R.make_operands(c, torch.float16, B, D, H, W, epilogue="bn_relu_skip")
        vox = R.skip_voxels(c, o["skip"].shape)
        R.poison_skip_and_bias(c, o, vox)
        r = R.reference(c, o, with_skip=True, floor=R.cycled_floor(c.c_out), relu_pre=pre, relu_post=post)
        y = r.y
        assert bool(torch.isnan(y[vox[2]]).all()) and bool((y[vox[1]] == INF).any())
        assert bool((y[vox[0]] == (0.0 if post else -INF)).all())
        if c.c_out > 1:
            ch = y[..., c.c_out - 1]
            fl = float(R.cycled_floor(c.c_out)[-1])
            keep = torch.ones_like(ch, dtype=torch.bool)
            for v in vox:
                keep[v] = False
            if pre:
                sk = o["skip"][..., c.c_out - 1].double()
                want = fl + sk
                want = torch.where(want < 0, torch.zeros_like(want), want) if post else want
                assert torch.equal(ch[keep], want[keep])
            else:
                assert bool((ch[keep] == (0.0 if post else -INF)).all())
