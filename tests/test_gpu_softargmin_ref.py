"""pscv_softargmin, pscv_softargmin_window and the fused siblings held to the float64 reference of tests/_softargmin_ref.py: every
kernel path (thread-per-pixel, register slices, two-pass slices), logit type, plane layout, confidence mode and edge the family
has.  The case table below is imported by tests/test_softargmin_ref_cpu.py, which checks it from float64 alone.

Both confidences are discontinuous in the expected index.  Where the float64 index lies within the index tolerance of such a
discontinuity (``Ref.fragile``), the kernel's value must equal the reference or the value on the other side; nothing is skipped.

Tolerances (``TOL``; DESIGN.md section 4 holds the measured table): 4 x the worst error measured over all cases of this file on an
MI355X, rounded up to one digit; units: index x (D + offset), depth x max |plane| (max |logit| for "depth := logits"), the rest
absolute.  16-bit logits use the same bounds: the reference sees the rounded logits."""
import collections
import json
import os

import numpy as np
import pytest
import torch

import _softargmin_ref as R

pytestmark = pytest.mark.gpu

TOL = {
    # output: bound            worst measured (family)        4 x worst
    "index": 3e-6,           # 6.03e-7 (slice)                2.4e-6      x (D + offset)
    "depth": 3e-6,           # 5.30e-7 (slice)                2.1e-6      x max |plane|
    "conf": 3e-6,            # 5.24e-7 (-inf planes)          2.1e-6
    "entropy": 8e-6,         # 1.91e-6 (regimes: sigma 0.01)  7.6e-6
    "prob": 1e-6,            # 5.19e-7 (slice)                2.1e-6: capped by the 1e-6 the golden test already held
    "z": 3e-6,               # 5.02e-7 (slice)                2.0e-6      relative, sum e of the partials
    # the fused sweeps (fast exponential, a running re-base per 6-plane block, per-chunk merge)
    "fused_depth": 9e-7,     # 2.06e-7 (prob_softargmin)      8.2e-7      x max |plane|
    "fused_conf": 1e-6,      # 2.30e-7 (tail_sweep)           9.2e-7
    "fused_index": 2e-6,     # 2.64e-7 (head_index_entropy)   1.06e-6     x D
    "fused_entropy": 2e-6,   # 3.64e-7 (head_index_entropy)   1.46e-6
}
FRAGILE_CAP = 0.03
GRIDS = [(2, 19, 27), (1, 3, 5)]        # 513 pixels per item: a 32-pixel workgroup straddles the batch seam, ragged end; < 1 workgroup
OFFSETS = [0, 96]
CONF = [(0, 2.0), (1, 2.0), (1, 2.5)]   # (conf_mode, window)
DTYPES = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}

Case = collections.namedtuple("Case", "family D dtype regime capped offsets")


def _cases():
    out = []
    for D in (1, 9, 41, 33, 40, 64, 192, 256, 257, 300):            # 1, 9, 41: empty trailing slices; 256 last register size; then two-pass
        for dt in DTYPES:
            out.append(Case("slice", D, dt, "normal", True, OFFSETS))
    for D in (1, 8, 9, 16, 17, 32, 33):                             # 33: the first size the thread-per-pixel kernel must not take
        out.append(Case("small", D, "fp32", "normal", True, OFFSETS))
    for D in (41, 257):
        for dt in DTYPES:
            out.append(Case("regime", D, dt, "flat", True, OFFSETS))
            out.append(Case("regime", D, dt, "peaked", False, OFFSETS))
            out.append(Case("regime", D, dt, "extreme", False, OFFSETS))
            out.append(Case("regime", D, dt, "constant", False, OFFSETS))
            out.append(Case("regime", D, dt, "near_integer", True, [0]))
    return out


CASES = _cases()
NEAR = 1e-3         # distance of the "near_integer" index from the integer


def case_id(c):
    return f"{c.family}-D{c.D}-{c.dtype}-{c.regime}"


def make_logits(c, grid, extra_seed=0):
    """CPU fp32 logits [B,D,h,w] holding values of the case's storage type."""
    B, h, w = grid
    D = c.D
    g = torch.Generator().manual_seed(1000 * D + 10 * len(c.regime) + h + extra_seed)
    if c.regime == "normal":
        l = torch.randn(B, D, h, w, generator=g) * 4
    elif c.regime == "flat":
        l = torch.randn(B, D, h, w, generator=g) * 0.01
    elif c.regime == "peaked":
        l = torch.randn(B, D, h, w, generator=g) * 30
    elif c.regime == "extreme":
        big = 6.0e4 if c.dtype == "fp16" else 3.0e4
        sign = (torch.rand(B, D, h, w, generator=g) < 0.5).float() * 2 - 1
        l = sign * big + torch.randn(B, D, h, w, generator=g) * 4
        l[:, 0] = l[:, 0].abs()                                    # (every column holds a plane at + big)
    elif c.regime == "constant":
        l = torch.full((B, D, h, w), 1.25)
    elif c.regime == "near_integer":
        # two planes i, i + 1 share the mass (1 - t, t), t = NEAR or 1 - NEAR: the index is i + t; the others lie 80 below
        i = torch.randint(0, D - 1, (B, 1, h, w), generator=g)
        below = torch.rand(B, 1, h, w, generator=g) < 0.5
        t = torch.where(below, torch.tensor(1.0 - NEAR), torch.tensor(NEAR)).double()
        l = torch.full((B, D, h, w), -80.0)
        l.scatter_(1, i, torch.zeros(B, 1, h, w))
        l.scatter_(1, i + 1, torch.log(t / (1 - t)).float())
    else:
        raise ValueError(c.regime)
    return l.to(DTYPES[c.dtype]).float().contiguous()


def make_planes(D, grid, per_pixel, seed=0):
    B, h, w = grid
    g = torch.Generator().manual_seed(77 + D + seed)
    if per_pixel:
        return (torch.rand(B, D, h, w, generator=g) + torch.arange(D).view(1, D, 1, 1) * 0.05 + 2.0).contiguous()
    return (torch.rand(B, 1, generator=g) + 1.5 + torch.arange(D).view(1, D) * (4.0 / max(D - 1, 1)) * (1 + torch.arange(B).view(B, 1))).contiguous()


def index_eps(D, offset, key="index"):
    return TOL[key] * (D + offset)


# ------------------------------------------------------------------------------------------------
WORST = {}          # (family, output) -> worst error in the output's unit


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from wild_deep_mvs_amd import _lib as L, ops
    yield L, ops
    print("\n[softargmin ref] worst error per case family and output (unit: see TOL):", flush=True)
    for (fam, name), v in sorted(WORST.items()):
        print(f"[softargmin ref]   {fam:14s} {name:14s} {v:.3e}", flush=True)
    path = os.environ.get("PSCV_SOFTARGMIN_ERR_TABLE")
    if path:
        with open(path, "w") as fh:
            json.dump({f"{fam}/{name}": v for (fam, name), v in sorted(WORST.items())}, fh, indent=1)


def _np(t_):
    return t_.detach().double().cpu().numpy()


def check(fam, name, got, ref, *, scale=1.0, tol=None, alts=None, mask=None, what=""):
    """|got - ref| / scale <= TOL[tol or name]; NaN exactly where the reference is NaN; at ``mask`` pixels any of ``alts`` will do."""
    got = _np(got) if torch.is_tensor(got) else np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    nan_ref = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan_ref), f"{fam} {name} {what}: NaN at {int(np.isnan(got).sum())} places, reference at {int(nan_ref.sum())}"
    with np.errstate(invalid="ignore"):
        err = np.abs(got - ref)
        for alt in alts or ():
            err = np.where(mask, np.minimum(err, np.abs(got - alt)), err)
    err = np.where(nan_ref, 0.0, err)
    worst = float(err.max()) / scale if err.size else 0.0
    WORST[(fam, name)] = max(WORST.get((fam, name), 0.0), worst)
    bound = TOL[tol or name]
    if worst > bound:
        k = np.unravel_index(int(err.argmax()), err.shape)
        raise AssertionError(f"{fam} {name} {what}: worst error {worst:.3e} x {scale:g} > {bound:.1e} x {scale:g} at {tuple(int(i) for i in k)}: "
                             f"got {got[k]!r}, reference {ref[k]!r}")
    return worst


def run_and_check(ops, fam, lg, planes, ref, *, offset, what, small_ok=False, want_prob=True, want_partials=True, depth_scale=None,
                  conf=CONF):
    """One launch per confidence mode with every output the kernel choice allows; everything against ``ref``.  Returns the outputs
    of the last launch."""
    D = ref.D
    o = None
    dscale = depth_scale if depth_scale is not None else (float(np.abs(ref.planes).max()) if planes is not None else 1.0)
    for mode, window in conf:
        o = ops.softargmin(lg, planes, want_index=True, want_conf=True, conf_mode=mode, window=window, want_entropy=True,
                           want_prob=want_prob and not small_ok, want_partials=want_partials and not small_ok, index_offset=offset)
        w_ = f"{what} mode {mode} window {window}"
        check(fam, "index", o["index"], ref.index, scale=D + offset, what=w_)
        if planes is not None:
            check(fam, "depth", o["depth"], ref.depth, scale=dscale, what=w_)
        check(fam, "entropy", o["entropy"], ref.entropy(), what=w_)
        mask, alts = ref.fragile(mode, index_eps(D, offset), window)
        check(fam, "conf", o["conf"], ref.conf(mode, window), alts=alts, mask=mask, what=w_)
        if "prob" in o:
            check(fam, "prob", o["prob"], ref.prob, what=w_)
        if "partials" in o:
            check_partials(fam, o["partials"], ref, dscale, what=w_)
    return o


def check_partials(fam, part, ref, dscale, what=""):
    """(max, sum e, sum e * depth, sum e * index): the max is exact, the sums as Z (relative) and as the depth / index they encode."""
    p = _np(part)
    want = ref.partials()
    live = np.isfinite(want[:, 0])
    assert np.array_equal(p[:, 0][live], want[:, 0][live]) and np.array_equal(np.isneginf(p[:, 0]), np.isneginf(want[:, 0])), f"{fam} partial max {what}"
    empty = np.isneginf(want[:, 0])
    assert (p[:, 1:][np.broadcast_to(empty[:, None], p[:, 1:].shape)] == 0).all(), f"{fam} {what}: an all -inf shard must hand (-inf, 0, 0, 0) on"
    ok = live & ~ref.bad
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.where(ok, np.abs(p[:, 1] - want[:, 1]) / np.where(ok, want[:, 1], 1.0), 0.0)
        check(fam, "z", rel, np.zeros_like(rel), what=what)
        check(fam, "index", np.where(ok, p[:, 3] / p[:, 1], 0.0), np.where(ok, ref.index, 0.0), scale=ref.D + ref.offset, what="partials " + what)
        if ref.planes is not None:
            check(fam, "depth", np.where(ok, p[:, 2] / p[:, 1], 0.0), np.where(ok, ref.depth, 0.0), scale=dscale, what="partials " + what)


# ------------------------------------------------------------------------------------------------
# the case table: slice kernel, thread-per-pixel kernel, logit regimes
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_case_table_against_float64(env, case):
    L, ops = env
    D = case.D
    for grid in GRIDS:
        lg_cpu = make_logits(case, grid)
        lg = lg_cpu.to(DTYPES[case.dtype]).cuda()
        assert torch.equal(lg.float().cpu(), lg_cpu)
        for per_pixel in (False, True):
            planes = make_planes(D, grid, per_pixel)
            for offset in case.offsets:
                ref = R.Ref(lg_cpu, planes, offset)
                what = f"{case_id(case)} grid {grid} per_pixel {per_pixel} offset {offset}"
                if case.family == "small":
                    with L.tuning(softargmin_small=1):
                        a = run_and_check(ops, "small", lg, planes.cuda(), ref, offset=offset, what=what, small_ok=True)
                    with L.tuning(softargmin_small=0):
                        b = run_and_check(ops, "slice", lg, planes.cuda(), ref, offset=offset, what=what, small_ok=True)
                    # both kernels against each other (last confidence mode: 1, window 2.5)
                    mask, _ = ref.fragile(1, index_eps(D, offset), 2.5)
                    for k, scale in (("depth", float(planes.abs().max())), ("index", D + offset), ("entropy", 1.0), ("conf", 1.0)):
                        d = (a[k] - b[k]).abs().double().cpu().numpy()
                        if k == "conf":
                            d = np.where(mask, 0.0, d)
                        assert float(d.max()) <= TOL[k] * scale, f"{what}: {k} of the two kernels differs by {float(d.max()):.3e}"
                    same = all(torch.equal(a[k], b[k]) for k in ("depth", "index", "entropy", "conf"))
                    if D > 32:
                        assert same, f"{what}: D > 32 must run the slice kernel whatever softargmin_small says"
                    elif D == 32 and grid == GRIDS[0]:
                        assert not same, f"{what}: softargmin_small = 1 at D = 32 did not change a bit: did the thread-per-pixel kernel run?"
                else:
                    with L.tuning(softargmin_small=0):
                        run_and_check(ops, case.family, lg, planes.cuda(), ref, offset=offset, what=what)


# ------------------------------------------------------------------------------------------------
# -inf planes, NaN
# ------------------------------------------------------------------------------------------------
def _neginf_logits(D, grid, kind, seed):
    B, h, w = grid
    g = torch.Generator().manual_seed(seed)
    l = torch.randn(B, D, h, w, generator=g) * 4
    if kind == "scattered":
        drop = torch.rand(B, D, h, w, generator=g) < 0.15
        drop[:, int(D // 2)] = False                                  # (no column loses every plane)
        l[drop] = float("-inf")
    else:                                                             # one whole depth slice of the slice kernel
        per = (D + 7) // 8
        sl = 3 if D > 3 * per else 0
        l[:, sl * per:min(D, (sl + 1) * per)] = float("-inf")
        l[0, :, 1, 2] = torch.randn(D, generator=g)                   # (one pixel keeps the slice, its neighbours do not)
    return l.contiguous()


@pytest.mark.parametrize("kind", ["scattered", "whole_slice"])
@pytest.mark.parametrize("D", [32, 64, 257])
def test_minus_infinity_planes_weigh_zero(env, D, kind):
    """torch.softmax semantics: a -inf logit has probability 0, the rest of the column is untouched.  "whole_slice" makes every plane
    of ONE of the slice kernel's eight depth slices -inf (D = 64: planes 24..31; D = 257: the two-pass loop's planes 99..131;
    D = 32: planes 12..15, also through the thread-per-pixel kernel): before the guard in softargmin_kernel that slice's
    exp(-inf - -inf) made the pixel NaN."""
    L, ops = env
    grid = GRIDS[0]
    lg_cpu = _neginf_logits(D, grid, kind, seed=D)
    for per_pixel in (False, True):
        planes = make_planes(D, grid, per_pixel)
        ref = R.Ref(lg_cpu, planes, 5)
        assert not ref.bad.any() and np.isfinite(ref.depth).all()
        for small in ((1, 0) if D <= 32 else (0,)):
            with L.tuning(softargmin_small=small):
                run_and_check(ops, "neginf", lg_cpu.cuda(), planes.cuda(), ref, offset=5, what=f"-inf {kind} D={D} small={small} per_pixel {per_pixel}",
                              small_ok=bool(small))


@pytest.mark.parametrize("D,small", [(16, 1), (16, 0), (41, 0), (257, 0)])
def test_nan_logit_poisons_its_pixel_only(env, D, small):
    L, ops = env
    grid = GRIDS[0]
    g = torch.Generator().manual_seed(3 + D)
    lg_cpu = (torch.randn(grid[0], D, grid[1], grid[2], generator=g) * 4).contiguous()
    lg_cpu[1, D // 3, 7, 11] = float("nan")
    lg_cpu[0, :, 2, 3] = float("-inf")                                # and a column without any finite logit
    planes = make_planes(D, grid, False)
    ref = R.Ref(lg_cpu, planes, 0)
    assert int(ref.bad.sum()) == 2
    with L.tuning(softargmin_small=small):
        o = ops.softargmin(lg_cpu.cuda(), planes.cuda(), want_index=True, want_entropy=True, want_prob=not small)
        for k, want in (("depth", ref.depth), ("index", ref.index), ("entropy", ref.entropy())):
            check("nan", k, o[k], want, scale=float(planes.max()) if k == "depth" else D if k == "index" else 1.0, what=f"NaN D={D}")
        if not small:
            check("nan", "prob", o["prob"], ref.prob, what=f"NaN D={D}")
        for mode, window in CONF:
            c = ops.softargmin(lg_cpu.cuda(), None, want_conf=True, conf_mode=mode, window=window)["conf"]
            mask, alts = ref.fragile(mode, index_eps(D, 0), window)
            check("nan", "conf", c, ref.conf(mode, window), alts=alts, mask=mask, what=f"NaN D={D} mode {mode}")


# ------------------------------------------------------------------------------------------------
# partials of uneven shards, merged on the host; the window probability per shard
# ------------------------------------------------------------------------------------------------
SHARDS = {192: (100, 57, 35), 257: (100, 57, 100)}


@pytest.mark.parametrize("planes_kind", ["shared", "per_pixel", "logits", "shard_minus_inf"])
@pytest.mark.parametrize("D", [192, 257])
def test_uneven_shards_merge_to_the_full_range(env, D, planes_kind):
    """Three uneven depth shards, each with its index offset: the partials merge (log-sum-exp, float64 on the host) into the
    full-range reference; "logits": depth := the logits, as the Vis depth-shard path calls it (model_cas.py `_merged_head`);
    "shard_minus_inf": the middle shard holds -inf only.  Then pscv_softargmin_window per shard under the merged statistics: the
    shard outputs sum to the window probability of the whole axis."""
    L, ops = env
    grid = GRIDS[0]
    g = torch.Generator().manual_seed(D + len(planes_kind))
    lg_cpu = (torch.randn(grid[0], D, grid[1], grid[2], generator=g) * 4).contiguous()
    sizes = SHARDS[D]
    bounds = np.concatenate([[0], np.cumsum(sizes)])
    if planes_kind == "shard_minus_inf":
        lg_cpu[:, bounds[1]:bounds[2]] = float("-inf")
    planes = lg_cpu if planes_kind == "logits" else make_planes(D, grid, planes_kind == "per_pixel")
    full = R.Ref(lg_cpu, planes, 0)
    dscale = float(planes.abs().max())
    parts, owns = [], []
    for a, b in zip(bounds[:-1], bounds[1:]):
        own = lg_cpu[:, a:b].contiguous()
        pl = planes[:, a:b].contiguous()
        sref = R.Ref(own, pl, int(a))
        o = ops.softargmin(own.cuda(), pl.cuda(), want_partials=True, index_offset=int(a))
        check_partials("shards", o["partials"], sref, dscale, what=f"shard [{a},{b}) of {D} {planes_kind}")
        parts.append(o["partials"])
        owns.append((own, int(a)))
    m = R.merge(parts)
    check("shards", "depth", m["depth"], full.depth, scale=dscale, what=f"merged {D} {planes_kind}")
    check("shards", "index", m["index"], full.index, scale=D, what=f"merged {D} {planes_kind}")
    np.testing.assert_array_equal(m["max"], full.m)
    stats = torch.from_numpy(np.stack([m["max"], m["z"], m["index"]], axis=1)).float().contiguous().cuda()
    for window in (2.0, 2.5):
        tot = sum(ops.softargmin_window(own.cuda(), stats, window=window, index_offset=a).double() for own, a in owns)
        mask, alts = full.fragile(1, index_eps(D, 0), window)
        check("shards", "conf", tot, full.conf1(window), alts=alts, mask=mask, what=f"window {window} of {D} {planes_kind}")


# ------------------------------------------------------------------------------------------------
# into=
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,small", [(16, 1), (41, 0)])
def test_into_writes_batch_slices_only(env, D, small):
    L, ops = env
    B, h, w = GRIDS[0]
    g = torch.Generator().manual_seed(D)
    lg = (torch.randn(B, D, h, w, generator=g) * 4).cuda()
    planes = make_planes(D, GRIDS[0], False).cuda()
    names = ("depth", "index", "conf", "entropy")
    with L.tuning(softargmin_small=small):
        fresh = ops.softargmin(lg, planes, want_index=True, want_conf=True, conf_mode=1, want_entropy=True)
        bufs = {k: torch.full((3 * B, h, w), -7.0, device="cuda") for k in names}
        got = ops.softargmin(lg, planes, want_index=True, want_conf=True, conf_mode=1, want_entropy=True,
                             into={k: bufs[k][B:2 * B] for k in names})
    for k in names:
        assert got[k].data_ptr() == bufs[k][B:2 * B].data_ptr()
        assert torch.equal(bufs[k][B:2 * B], fresh[k]), k
        assert bool((bufs[k][:B] == -7.0).all()) and bool((bufs[k][2 * B:] == -7.0).all()), f"{k}: a neighbouring batch slice was written"
    with pytest.raises(ValueError):
        ops.softargmin(lg, planes, into={"index": bufs["index"][B:2 * B]})           # not requested
    with pytest.raises(ValueError):
        ops.softargmin(lg, planes, want_index=True, into={"index": bufs["index"]})   # wrong shape


# ------------------------------------------------------------------------------------------------
# argument errors
# ------------------------------------------------------------------------------------------------
def test_argument_errors_raise_instead_of_launching(env):
    L, ops = env
    lg = torch.zeros(1, 8, 3, 5, device="cuda")
    dv = torch.ones(1, 8, device="cuda")
    with pytest.raises(L.PscvError, match="conf_mode"):
        ops.softargmin(lg, dv, want_conf=True, conf_mode=2)
    with pytest.raises(ValueError):
        ops.softargmin(lg, dv.double())
    with pytest.raises(ValueError):
        ops.softargmin(lg, torch.ones(1, 7, device="cuda"))
    with pytest.raises(ValueError):
        ops.softargmin(lg[0], dv)
    with pytest.raises(TypeError):
        ops.softargmin(lg.double(), dv)
    with pytest.raises(RuntimeError):
        ops.softargmin(lg.cpu(), dv.cpu())
    out = torch.full((1, 3, 5), -7.0, device="cuda")
    rc = L.lib().pscv_softargmin(lg.data_ptr(), L.F32, None, 0, 0, out.data_ptr(), None, None, None, None, None, 0, 2.0, 0, 1, 8, 3, 5, None)
    assert rc != 0 and "out_depth requested without depth planes" in L.lib().pscv_last_error().decode()
    rc = L.lib().pscv_softargmin(lg.data_ptr(), 99, dv.data_ptr(), 8, 0, out.data_ptr(), None, None, None, None, None, 0, 2.0, 0, 1, 8, 3, 5, None)
    assert rc != 0 and "bad logit dtype" in L.lib().pscv_last_error().decode()
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())


# ------------------------------------------------------------------------------------------------
# fused siblings: their own fp32 logits (pinned bit for bit to conv3d elsewhere) -> the float64 reference of those logits
# ------------------------------------------------------------------------------------------------
def _bf16r(x):
    return x.to(torch.bfloat16).float()


def _check_fused_regression(fam, fz, dv, what):
    """depth and the 4-plane confidence of a fused tail against the reference of the logits it returned.  The index the confidence
    truncates is not an output: the caller's second launch with the planes 0 .. D-1 returns it as "depth" (the same sums)."""
    lg = fz["logits"].float().cpu()
    D = lg.shape[1]
    ref = R.Ref(lg, dv.cpu(), 0)
    check(fam, "fused_depth", fz["depth"], ref.depth, scale=float(dv.abs().max()), what=what)
    mask, alts = ref.fragile(0, TOL["fused_index"] * D)
    check(fam, "fused_conf", fz["conf"], ref.conf0(), alts=alts, mask=mask, what=what)
    assert float(mask.mean()) <= FRAGILE_CAP, f"{what}: {float(mask.mean()):.3f} of the pixels are fragile"
    return ref


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("D,one_chunk", [(18, False), (37, False), (37, True)])
def test_fused_prob_softargmin_against_float64(env, D, one_chunk, dtype):
    """pscv_prob_softargmin (conv3d_c1.hip FUSE 1 + softargmin_merge_kernel): 9 x 40 pixels, batch of two with different planes, one
    6-plane block per chunk (3 / 7 chunks) and the whole axis in one chunk; a second call with the planes 0 .. D-1 exposes the index."""
    L, ops = env
    H, W = 9, 40
    g = torch.Generator().manual_seed(61 + D)
    x = _bf16r(torch.randn(2, 8, D, H, W, generator=g))
    w = _bf16r(torch.randn(1, 8, 3, 3, 3, generator=g) * 1.5 / np.sqrt(27 * 8))
    dv = torch.stack([torch.linspace(2.0, 6.0, D), torch.linspace(1.0, 9.0, D)]).cuda().contiguous()
    ar = torch.arange(D, dtype=torch.float32).repeat(2, 1).cuda().contiguous()
    layer = ops.Conv3dLayer.build(w, kind=L.CONV_S1, device="cuda", conv_bias=torch.randn(1, generator=g), dtype=dtype)
    xcl = ops.to_channels_last(x.cuda(), dtype)
    with L.tuning(c1_sweep=2, c1_nb=8 if one_chunk else 0):
        fz = ops.prob_softargmin(xcl, layer, dv)
        fi = ops.prob_softargmin(xcl, layer, ar, want_conf=False)
    assert fz is not None and fi is not None and torch.equal(fz["logits"], fi["logits"])
    ref = _check_fused_regression("fused_prob", fz, dv, f"prob_softargmin D={D} one_chunk={one_chunk} {dtype}")
    check("fused_prob", "fused_index", fi["depth"], ref.index, scale=D, what=f"prob_softargmin index D={D}")


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("nbk", [1, 0])
@pytest.mark.parametrize("shape", [(9, 4, 14), (13, 12, 30)])
def test_tail_sweep_regression_against_float64(env, shape, nbk, dtype):
    """pscv_tail_sweep(regress=...): the statistics kept by the sweep and its merge launch; tail_nbk = 1: one 6-plane block per chunk
    (3 / 5 chunks), 0: the default chunking."""
    L, ops = env
    Di, Hi, Wi = shape
    B = 2
    g = torch.Generator().manual_seed(17 + sum(shape))
    x = _bf16r(torch.randn(B, 16, Di, Hi, Wi, generator=g))
    wu = _bf16r(torch.randn(16, 8, 3, 3, 3, generator=g) / np.sqrt(27 * 16 / 8))
    wh = _bf16r(torch.randn(1, 8, 3, 3, 3, generator=g) * 1.5 / np.sqrt(27 * 8))
    bn = (torch.rand(8, generator=g) + 0.5, torch.randn(8, generator=g) * 0.1, torch.randn(8, generator=g) * 0.1, torch.rand(8, generator=g) + 0.5)
    skip = _bf16r(torch.randn(B, 8, 2 * Di, 2 * Hi, 2 * Wi, generator=g))
    up = ops.Conv3dLayer.build(wu, kind=L.CONV_T2, transposed=True, device="cuda", bn=bn, relu=True, dtype=dtype)
    head = ops.Conv3dLayer.build(wh, kind=L.CONV_S1, device="cuda", conv_bias=torch.randn(1, generator=g), dtype=dtype)
    D2 = 2 * Di
    dv = torch.stack([torch.linspace(2.0, 6.0, D2), torch.linspace(1.0, 9.0, D2)]).cuda().contiguous()
    ar = torch.arange(D2, dtype=torch.float32).repeat(2, 1).cuda().contiguous()
    xcl, scl = ops.to_channels_last(x.cuda(), dtype), ops.to_channels_last(skip.cuda(), dtype)
    with L.tuning(tail_nbk=nbk):
        fz = ops.tail_sweep(xcl, up, head, skip=scl, regress=dv)
        fi = ops.tail_sweep(xcl, up, head, skip=scl, regress=ar, want_conf=False)
    assert isinstance(fz, dict) and isinstance(fi, dict) and torch.equal(fz["logits"], fi["logits"])
    ref = _check_fused_regression("fused_tail", fz, dv, f"tail_sweep {shape} tail_nbk={nbk} {dtype}")
    check("fused_tail", "fused_index", fi["depth"], ref.index, scale=D2, what=f"tail_sweep index {shape}")


CLAMP_EFFECT = {}


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("D,one_chunk", [(16, True), (16, False), (37, False), (37, True)])
def test_head_index_entropy_against_float64(env, D, one_chunk, dtype):
    """pscv_head_index_entropy (conv3d_c1.hip FUSE 2): D = 16 in one chunk is written by the sweep itself, several chunks go through
    index_entropy_merge_kernel.  The fused entropy is log Z - E[logit - max] without the reference's clamp of p at 1e-9: held to the
    clamped reference at the bound, and the difference the clamp makes (float64, these logits) is printed."""
    L, ops = env
    B, H, W = 2, 9, 40
    g = torch.Generator().manual_seed(D * 100 + W)
    x = (torch.randn(B, D, H, W, 8, generator=g) * 2.0).to(dtype).cuda()
    w = _bf16r(torch.randn(1, 8, 3, 3, 3, generator=g) * 0.3)                          # logits over +-15: peaked and flat pixels
    layer = ops.Conv3dLayer.build(w, kind=L.CONV_S1, device="cuda", dtype=dtype)
    idx = torch.empty(B, H, W, device="cuda")
    ent = torch.empty(B, H, W, device="cuda")
    with L.tuning(c1_sweep=2, c1_nb=8 if one_chunk else 0):
        score = ops.head_index_entropy(x, layer, idx, ent, want_scores=True)
    assert score is not None and score is not True
    ref = R.Ref(score.float().cpu(), None, 0)
    what = f"head_index_entropy D={D} one_chunk={one_chunk} {dtype}"
    check("fused_head", "fused_index", idx, ref.index, scale=D, what=what)
    check("fused_head", "fused_entropy", ent, ref.entropy(), what=what)
    check("fused_head", "fused_entropy", ent, ref.entropy(clamp=False), what=what + " (no clamp)")
    eff = float(np.abs(ref.entropy() - ref.entropy(clamp=False)).max())
    CLAMP_EFFECT[what] = eff
    print(f"[softargmin ref] {what}: the clamp of p at 1e-9 changes the float64 entropy by at most {eff:.3e}", flush=True)
    assert eff <= TOL["fused_entropy"], "these logits were meant to keep the clamp's effect below the entropy bound"
