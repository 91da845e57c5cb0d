"""GPU: csrc/patch_match.hip against the float64 rule with the derived bounds of tests/_patch_match_bounds.py, on the cases of
tests/_patch_match_cases.py (17x33, 16x32, 40x56, 5x7, 1x40; n_src 1, 3, 4, 5, 31; a half-resolution and a 2x2 source; windows
(5,1), (8,1), (8,2), (4,4), (1,1); top_k 1, 2, 3, 8 and n_src).  Per entry and per decision, no pixel exempt as a whole:

  cost      c == 2 exactly where the source is decidedly invalid; |c - c_ref| <= bound on every valid decided entry; e_s inside its
            bound, exactly e_max where decidedly capped or invalid; agg equal to the mean of the kernel's own top_k smallest values
            and inside the propagated bound of the reference; non-finite and non-positive hypotheses in the same launch
  init      per-element bound
  half      candidates inside per-element bounds, skipped ones on every decided ``live``, the other colour untouched bit for bit,
            the written state bit-equal to the chosen candidate, the choice by regret at every pixel of the colour, the tie rule
            exactly, the reference's index where its best two are separated by more than their bounds
  filter    per-source decisions through the count: equal on every pixel whose sources are all decided, inside [passing,
            passing + undecided] everywhere; depth and normal are the state's bits where kept and 0 elsewhere; d <= 0 never kept
  twice     bit-identical on the default stream and on a side stream
tests/test_patch_match_ref_cpu.py applies the same checks to the fp32 emulation and plants the errors they must catch."""
import numpy as np
import pytest
import torch

from tests import _patch_match_bounds as PB
from tests import _patch_match_cases as CS
from tests import _patch_match_ref as PR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from wild_deep_mvs_amd import _lib as L, ops
    L.lib()
    return ops


def _dev(c, geometric):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t(c.ref), [t(s) for s in c.srcs], t(c.cams), ([t(d) for d in c.sdepths] if geometric else None)


def _cost(ops, name, geometric):
    c = CS.case(name)
    ref, srcs, cams, sd = _dev(c, geometric)
    cost, err, agg = ops.patch_match_cost(torch.from_numpy(c.state).cuda(), ref, srcs, cams, src_depths=sd, radius=c.radius, step=c.step,
                                          top_k=c.top_k)
    assert (err is None) == (not geometric)
    return cost.cpu().numpy(), None if err is None else err.cpu().numpy(), agg.cpu().numpy()


def _half(ops, name, geometric, colour, converged):
    c = CS.case(name)
    ref, srcs, cams, sd = _dev(c, geometric)
    st = torch.from_numpy(CS.half_state(c, converged)).cuda()
    choice, cand = ops.patch_match_half_step(st, ref, srcs, cams, c.dmin, c.dmax, src_depths=sd, radius=c.radius, step=c.step,
                                             top_k=c.top_k, want_choice=True, want_candidates=True, **CS.half_args(c, geometric, colour))
    return st.cpu().numpy(), choice.cpu().numpy(), cand.cpu().numpy()


def _filter(ops, name):
    c = CS.case(name)
    ref, srcs, cams, sd = _dev(c, True)
    d, n, cnt = ops.patch_match_filter(torch.from_numpy(c.state).cuda(), ref, srcs, cams, sd, radius=c.radius, step=c.step, want_count=True)
    return d.cpu().numpy(), n.cpu().numpy(), cnt.cpu().numpy()


@pytest.mark.parametrize("geometric", [False, True])
@pytest.mark.parametrize("name", CS.COST_CASES + ["grazing16x32"])
def test_cost_per_entry(ops, name, geometric):
    got = _cost(ops, name, geometric)
    res, sh = CS.verify_cost(name, geometric, *got)
    print("\n" + PB.fmt(f"{name} {'geometric' if geometric else 'photometric'}", res), sh)
    assert not PB.failures(res)
    assert res["flag"][1] > 0 and res["agg"][1] == got[2].size


def test_edge_hypotheses_in_the_same_launch(ops):
    """d in {0, negative, NaN, +inf}, a zero normal and a normal facing away, each between two ordinary pixels: the rule's
    definitions hold (fmaxf maps NaN to 0, a tap behind samples (0, 0)) and nothing leaks into the neighbours."""
    name = "exact16x32+edges"
    c = CS.case(name)
    cm, gm = CS.cost_models(name)
    cost, err, agg = _cost(ops, name, True)
    cost, err = cost.reshape(c.S, -1), err.reshape(c.S, -1)
    for key, (r, col) in c.edge_pixels.items():
        for p in (r * c.w + col - 1, r * c.w + col, r * c.w + col + 1):
            assert cm["vdec"][:, p].all() or p != r * c.w + col, key
            dec = cm["vdec"][:, p]
            assert np.array_equal((cost[:, p] == 2.0)[dec], ~cm["valid"][:, p][dec]), key
            ok = dec & cm["valid"][:, p]
            assert (np.abs(cost[:, p] - cm["c"][:, p])[ok] <= cm["cb"][:, p][ok] * PB.SCALE["cost"]).all(), key
            ex = gm["dec"][:, p] & gm["exact3"][:, p]
            assert (err[:, p][ex] == PR.GEOM_EMAX).all(), key
        if key in ("d=0", "d=nan", "d=inf", "n=0"):
            assert (cost[:, r * c.w + col] == 2.0).all(), key
    assert np.isfinite(agg).all()
    d, n, cnt = _filter(ops, name)
    for key in ("d=0", "d<0", "d=nan"):
        r, col = c.edge_pixels[key]
        assert d[r, col] == 0 and cnt[r, col] == 0 and (n[r, col] == 0).all(), key


def test_init_per_element(ops):
    for name in ("ragged17x33", "tiny5x7", "row1x40"):
        c = CS.case(name)
        v, b, dec = PB.init_model(c.h, c.w, c.cams, c.dmin, c.dmax, 5, 7)
        got = ops.patch_match_init(c.h, c.w, torch.from_numpy(c.cams).cuda(), c.dmin, c.dmax, seed=5, view=7).cpu().numpy()
        r = PB._ratio(np.abs(got - v), b * PB.SCALE["init"], dec[..., None] & np.ones(4, bool))
        print(f"\n[pm-ref] init {name}: {r}, flip undecided {1 - dec.mean():.2e}")
        assert r[0] == 0


@pytest.mark.parametrize("name,geometric,colour,converged", CS.HALF_CASES)
def test_half_step_per_pixel(ops, name, geometric, colour, converged):
    res, info = CS.verify_half(name, geometric, colour, converged, *_half(ops, name, geometric, colour, converged))
    print("\n" + PB.fmt(f"{name} g={geometric} colour={colour} converged={converged}", res), info)
    assert not PB.failures(res)
    assert res["regret"][1] == res["tie"][1] == len(PR.colour_pixels(CS.case(name).h, CS.case(name).w, colour)[0])


@pytest.mark.parametrize("name", CS.FILTER_CASES)
def test_filter_per_source(ops, name):
    res, info = CS.verify_filter(name, *_filter(ops, name))
    print("\n" + PB.fmt(name, res), info)
    assert not PB.failures(res)


def test_twice_is_bit_identical_on_both_streams(ops):
    name = "ragged17x33"

    def run():
        return [x for x in _cost(ops, name, True)] + list(_half(ops, name, True, 0, False)) + list(_filter(ops, name))
    a = run()
    b = run()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s = run()
    side.synchronize()
    for x, y, z in zip(a, b, s):
        assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)
        assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, z.view(np.uint32) if z.dtype == np.float32 else z)
