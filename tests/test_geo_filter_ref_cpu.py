"""The float64 reference of tests/_geo_filter_ref.py, checked WITHOUT a GPU:
  * the fp32 oracle (oracle/filtering.py, applied per source) agrees with it on every DECIDED (source, pixel, criterion) -- the band
    is wide enough for an independent fp32 evaluation in another operation order -- on both goldens and every scene of the GPU test;
  * the band is narrow enough: at most UNDECIDED_CAP = 1 % of the triples of any case are undecided, and no pixel is exempt as a whole;
  * the masks it implies equal the reference project's own masks (tests/golden/filter_*.npz) wherever every source is decided;
  * each planted error flips decided pairs: align_corners=True sampling, normalising by size, dropping the +1e-6, min for max, an
    angle left in radians, need = num_consistent."""
import numpy as np
import pytest
import torch

import _geo_filter_ref as GR
from _util import load_golden
from oracle import filtering as OF
from test_oracle_filter import golden_inputs

GOLDENS = ("filter_tiny.npz", "filter_upsample.npz")
_cache = {}


def scene_of(name):
    """(scene dict, list of (num_consistent, params))"""
    if name not in _cache:
        if name in GOLDENS:
            g = load_golden(name)
            depth, src, K, R, tt, nc = golden_inputs(g)
            sc = {"depth": depth, "src_depth": src, "K": K, "R": R, "t": tt, "golden": g}
            _cache[name] = (sc, ((nc, tuple(float(x) for x in g["params"])),))
        else:
            _cache[name] = (GR.make_case(name), GR.PARAMS)
    return _cache[name]


def ref_of(name, p):
    key = (name, p)
    if key not in _cache:
        _cache[key] = GR.reference(scene_of(name)[0], p)
    return _cache[key]


def oracle_pairs(sc, p):
    """the oracle's decisions per source: it is called with ONE source, num_consistent = 2, so its counts are the decisions"""
    N = len(sc["src_depth"])
    out = {k: [] for k in ("disp", "depth", "tri", "geo")}
    for i in range(N):
        sel = [0, i + 1]
        K, R, t = sc["K"][sel], sc["R"][sel], sc["t"][sel]
        m = OF.geometric_masks(sc["depth"], [sc["src_depth"][i]], K, R, t, max_reproj_error=p[0], depth_threshold=p[1],
                               min_tri_angle=p[2], num_consistent=2)
        q = OF.geometric_quantities(sc["depth"], [sc["src_depth"][i]], K, R, t)
        out["disp"].append(m["count_disp"].numpy() > 0)
        out["depth"].append(m["count_depth"].numpy() > 0)
        out["geo"].append(m["count_geo"].numpy() > 0)
        out["tri"].append((q["tri_angle"] > p[2])[0].numpy())
    return {k: np.stack(v) for k, v in out.items()}


@pytest.mark.parametrize("name", GOLDENS + GR.GPU_CASES)
def test_oracle_agrees_on_every_decided_pair_and_the_band_is_narrow(name):
    sc, plist = scene_of(name)
    for nc, p in plist:
        r = ref_of(name, p)
        o = oracle_pairs(sc, p)
        for k in ("disp", "depth", "tri", "geo"):
            bad = (o[k] != r[k]) & r[k + "_decided"]
            assert int(bad.sum()) == 0, f"{name} {p} {k}: the oracle differs on {int(bad.sum())} decided pairs, first {np.argwhere(bad)[:3].tolist()}"
        share, geo_share = GR.undecided_share(r)
        per = {k: float(1.0 - r[k + '_decided'].mean()) for k in GR.CRITERIA}
        print(f"[parity] geo filter ref {name} {p}: undecided {share:.3e} of the triples ({per}), geo {geo_share:.3e}", flush=True)
        assert share <= GR.UNDECIDED_CAP and geo_share <= GR.UNDECIDED_CAP, (name, p, share, geo_share)
        for k in GR.CRITERIA:                       # no criterion hides behind the other two
            assert per[k] <= GR.UNDECIDED_CAP, (name, p, k, per[k])


@pytest.mark.parametrize("name", GOLDENS)
def test_reference_masks_equal_the_reference_projects_own(name):
    sc, ((nc, p),) = scene_of(name)
    c, dec = GR.counts(ref_of(name, p))
    g = sc["golden"]
    for i, key in enumerate(("mask_depth", "mask_disp", "geo_mask")):
        want = np.asarray(g[key]).astype(bool)
        bad = ((c[i] >= nc - 1) != want) & dec[i]
        assert int(bad.sum()) == 0, f"{name} {key}: {int(bad.sum())} fully decided pixels differ"
        assert float(dec[i].mean()) > 0.95, (name, key, float(dec[i].mean()))


PLANT_SCENE = {"align_corners": "9v-96x128", "norm_size": "9v-96x128", "no_eps": "micro-scale", "min_for_max": "9v-96x128",
               "radians": "9v-96x128"}


@pytest.mark.parametrize("variant", [v for v in GR.VARIANTS if v])
def test_planted_error_flips_decided_pairs(variant):
    name = PLANT_SCENE[variant]
    sc, plist = scene_of(name)
    nc, p = plist[0]
    r = ref_of(name, p)
    cams = GR.cam_blocks(sc["K"], sc["R"], sc["t"])
    wrong = GR.pairs(sc["depth"].numpy(), [s.numpy() for s in sc["src_depth"]], cams, p, variant=variant)
    key = {"radians": "tri", "min_for_max": "depth", "no_eps": "depth"}.get(variant)
    flips = {k: int(((wrong[k] != r[k]) & r[k + "_decided"]).sum()) for k in ("disp", "depth", "tri", "geo")}
    print(f"[parity] geo filter ref planted {variant} on {name}: flipped decided pairs {flips}", flush=True)
    if key:
        assert flips[key] > 0, (variant, flips)
    else:
        assert flips["disp"] > 0 and flips["depth"] > 0, (variant, flips)


def test_planted_need_flips_fully_decided_pixels():
    name = "9v-96x128"
    sc, plist = scene_of(name)
    nc, p = plist[0]
    c, dec = GR.counts(ref_of(name, p))
    for i, key in enumerate(("mask_depth", "mask_disp", "geo_mask")):
        flipped = ((c[i] >= nc) != (c[i] >= nc - 1)) & dec[i]
        assert int(flipped.sum()) > 0, key


def test_certain_failures_are_decided():
    """A sample that leaves the source map reads depth 0: z' is ~1e-6 and may straddle 0, yet the reprojection error is in the thousands
    and the depth test fails whichever way the sign falls -- such pairs are decided.  Non-finite pairs are decided false."""
    sc, plist = scene_of("9v-96x128")
    nc, p = plist[0]
    r = ref_of("9v-96x128", p)
    q = OF.geometric_quantities(sc["depth"], sc["src_depth"], sc["K"], sc["R"], sc["t"])
    off = (q["warped_depth"] == 0).numpy() & (q["proj_depth_in_src"] > 0).numpy()
    assert int(off.sum()) > 500, int(off.sum())
    for k in ("disp", "depth", "geo"):
        assert float(r[k + "_decided"][off].mean()) > 0.99 and not r[k][off & r[k + "_decided"]].any(), k
    sc, plist = scene_of("non-finite")
    r = ref_of("non-finite", plist[0][1])
    bad = ~np.isfinite(sc["depth"].numpy())
    assert int(bad.sum()) == 8 and np.isnan(sc["depth"].numpy()).sum() == 4
    for k in ("disp", "depth", "geo"):
        assert r[k + "_decided"][:, bad].all() and not r[k][:, bad].any(), k
    zero = sc["depth"].numpy() == 0
    assert r["depth_decided"][:, zero].all() and not r["depth"][:, zero].any() and r["geo_decided"][:, zero].all()
    sc, plist = scene_of("pure-rotation")
    r = ref_of("pure-rotation", plist[0][1])
    fin = np.isfinite(sc["depth"].numpy())
    assert r["tri_decided"][:, fin].all() and not r["tri"][:, fin].any()
