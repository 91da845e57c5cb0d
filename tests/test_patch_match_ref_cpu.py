"""CPU: the error model of tests/_patch_match_bounds.py against the fp32 emulation of csrc/patch_match.hip
(tests/_patch_match_emu.py) on the cases of tests/_patch_match_cases.py -- the checks the GPU file applies to the kernel.

The emulation must lie inside every bound on every decided entry (the model is not too tight); the undecided shares and the
share of vacuous cost bounds are capped per case (the model decides almost everything); each planted error must be caught."""
import numpy as np
import pytest

from tests import _patch_match_bounds as PB
from tests import _patch_match_cases as CS
from tests import _patch_match_emu as EM
from tests import _patch_match_ref as PR

CAP = 0.01             # undecided (source, pixel, criterion) triples, e_s roundings and live decisions per case
VACUOUS_CAP = 0.02     # entries whose cost bound exceeds 1e-3, outside the grazing case


def _emu_cost(name, geometric, plant=None):
    c = CS.case(name)
    return EM.evaluate(c.ref, c.srcs, c.cams, c.rows, c.cols, c.state.reshape(-1, 4), c.radius, c.step, c.top_k,
                       c.sdepths if geometric else None, plant)[:3]


def _emu_half(name, geometric, colour, converged, plant=None):
    c = CS.case(name)
    new, best, cand = EM.half_step(CS.half_state(c, converged), c.ref, c.srcs, c.cams, c.dmin, c.dmax,
                                   src_depths=c.sdepths if geometric else None, radius=c.radius, step=c.step, top_k=c.top_k,
                                   plant=plant, **CS.half_args(c, geometric, colour))
    rows, cols = PR.colour_pixels(c.h, c.w, colour)
    choice = np.full((c.h, c.w), -1, np.int64)
    choice[rows, cols] = best
    cd = np.zeros((c.h, c.w, PR.NUM_CAND, 4), np.float32)
    cd[rows, cols] = cand
    return new, choice, cd


def _emu_filter(name, plant=None):
    c = CS.case(name)
    return EM.filter_state(c.state, c.ref, c.srcs, c.cams, c.sdepths, c.radius, c.step, plant)


@pytest.mark.parametrize("name", CS.COST_CASES)
def test_model_restates_the_reference(name):
    """The model's values are those of tests/_patch_match_ref.py (it only adds the bounds)."""
    c = CS.case(name)
    cm, gm = CS.cost_models(name)
    st = c.state.reshape(-1, 4).astype(np.float64)
    with np.errstate(all="ignore"):
        oc, _, _, _ = PR.source_costs(c.ref, c.srcs, c.cams, c.rows, c.cols, st[:, 0], st[:, 1:], c.radius, c.step)
        oe, _ = PR.geom_errors(c.cams, c.sdepths, c.rows, c.cols, st[:, 0], st[:, 1:])
    assert np.abs(oc - cm["c"])[cm["vdec"]].max() <= 1e-9
    assert np.abs(oe - gm["e"])[gm["dec"]].max() <= 1e-9


@pytest.mark.parametrize("geometric", [False, True])
@pytest.mark.parametrize("name", CS.COST_CASES)
def test_cost_emulation_inside_bounds_and_caps(name, geometric):
    res, sh = CS.verify_cost(name, geometric, *_emu_cost(name, geometric))
    print("\n" + PB.fmt(f"{name} {'geometric' if geometric else 'photometric'}", res), sh)
    assert not PB.failures(res)
    assert sh["undecided"] <= CAP and sh["e_undecided"] <= CAP and sh["vacuous"] <= VACUOUS_CAP
    assert res["cost"][1] > 0


def test_grazing_planes_get_a_larger_bound_not_an_exemption():
    name = "grazing16x32"
    c = CS.case(name)
    for geometric in (False, True):
        res, sh = CS.verify_cost(name, geometric, *_emu_cost(name, geometric))
        print("\n" + PB.fmt(name, res), sh)
        assert not PB.failures(res) and res["cost"][1] > 0.5 * c.S * c.h * c.w


def test_edge_hypotheses_are_decided():
    """d in {0, NaN, +inf} and a zero normal make every source decidedly invalid (c = 2, e_s by its own rule); a negative depth and a
    normal facing away are ordinary planes of the rule; the pixels next to them are ordinary."""
    c = CS.case("exact16x32+edges")
    cm, gm = CS.cost_models("exact16x32+edges")
    for key, (r, col) in c.edge_pixels.items():
        p = r * c.w + col
        assert cm["vdec"][:, p].all(), key
        if key in ("d=0", "d=nan", "d=inf", "n=0"):
            assert not cm["valid"][:, p].any(), key
        if key in ("d=0", "d<0", "d=nan"):
            assert (gm["dec"][:, p] & gm["exact3"][:, p]).all(), key
        assert cm["valid"][:, [p - 1, p + 1]].any(), key


def test_init_emulation_inside_bounds():
    c = CS.case("ragged17x33")
    v, b, dec = PB.init_model(c.h, c.w, c.cams, c.dmin, c.dmax, 5, 7)
    got = EM.random_hyp(c.cams, c.rows, c.cols, c.w, c.dmin, c.dmax, 5, 7, PR.INIT_ITERATION, 0).reshape(c.h, c.w, 4)
    r = PB._ratio(np.abs(got - v), b * PB.SCALE["init"], dec[..., None] & np.ones(4, bool))
    print(f"\n[pm-ref] init: {r}")
    assert r[0] == 0 and dec.mean() >= 1 - CAP
    assert np.abs(v - PR.init_state(c.h, c.w, c.cams, c.dmin, c.dmax, 5, 7)).max() <= 1e-9


@pytest.mark.parametrize("name,geometric,colour,converged", CS.HALF_CASES)
def test_half_step_emulation(name, geometric, colour, converged):
    res, info = CS.verify_half(name, geometric, colour, converged, *_emu_half(name, geometric, colour, converged))
    print("\n" + PB.fmt(f"{name} g={geometric} colour={colour} converged={converged}", res), info)
    assert not PB.failures(res)
    assert info["live_undecided"] <= CAP and info["branch_undecided"] <= CAP


@pytest.mark.parametrize("name", CS.FILTER_CASES)
def test_filter_emulation(name):
    res, info = CS.verify_filter(name, *_emu_filter(name))
    print("\n" + PB.fmt(name, res), info)
    assert not PB.failures(res) and info["filter_undecided"] <= CAP


# plant -> (what runs, the checks that must report violations)
PLANTED = {
    "noclamp": (lambda p: CS.verify_cost("ragged17x33", False, *_emu_cost("ragged17x33", False, p))[0], ("cost",)),
    "nocolour": (lambda p: CS.verify_cost("ragged17x33", False, *_emu_cost("ragged17x33", False, p))[0], ("cost",)),
    "cov": (lambda p: CS.verify_cost("ragged17x33", False, *_emu_cost("ragged17x33", False, p))[0], ("cost",)),
    "centre_rm": (lambda p: CS.verify_cost("rm-edge8x16", False, *_emu_cost("rm-edge8x16", False, p))[0], ("cost", "flag")),
    "half_even": (lambda p: CS.verify_cost("dyadic8x16", True, *_emu_cost("dyadic8x16", True, p))[0], ("err",)),
    "nocap": (lambda p: CS.verify_cost("ragged17x33", True, *_emu_cost("ragged17x33", True, p))[0], ("err3",)),
    "mean_all": (lambda p: CS.verify_cost("ragged17x33", False, *_emu_cost("ragged17x33", False, p))[0], ("topk", "agg")),
    "dist2": (lambda p: CS.verify_half("ragged17x33", False, 0, False, *_emu_half("ragged17x33", False, 0, False, p))[0], ("cand", "live")),
    "tie_high": (lambda p: CS.verify_half("dyadic8x16", False, 0, True, *_emu_half("dyadic8x16", False, 0, True, p))[0], ("tie",)),
    "axis": (lambda p: CS.verify_half("ragged17x33", False, 0, False, *_emu_half("ragged17x33", False, 0, False, p))[0], ("cand",)),
    "cos1": (lambda p: CS.verify_filter("dyadic8x16", *_emu_filter("dyadic8x16", p))[0], ("count", "range")),
}


@pytest.mark.parametrize("plant", EM.PLANTS)
def test_planted_error_is_caught(plant):
    """Each planted error must push decided entries outside their bound, flip decided decisions or change checked choices.

    ``centre_rm``: a shift of the centre sample is a common offset of the window's source values, to which the NCC is invariant,
    and 1.5 ulp of a position lies inside any valid cost bound; what it can change is the inside test of the centre.  The
    rm-edge case puts the centre exactly on the source's last column with every step exact in fp32, so the decision is decided:
    the quotient is inside, the reciprocal-multiply product one ulp outside, and the flags of that column flip."""
    run, names = PLANTED[plant]
    res = run(plant)
    caught = {k: res[k][0] for k in names if k in res}
    print("\n" + PB.fmt(f"planted {plant}", res), "caught:", caught)
    assert sum(caught.values()) > 0
