"""CPU: the float64 reference with derived bounds of the depth-map fusion (tests/_fusion_bounds.py) against the fp32 emulation of the
kernel (tests/_fusion_emu.py) on every case of tests/_fusion_cases.py: the emulation lies inside every bound and agrees on every
decided decision; every planted error is caught in a named case; at most 1 % of a case's (pass, source view, pixel, criterion)
tuples are undecided; the two dyadic cases are exact step by step; the colour rule holds for every sum and count."""
import numpy as np
import pytest

from tests import _fusion_bounds as FB
from tests import _fusion_cases as FC
from tests import _fusion_emu as EM
from tests import _fusion_ref as FR

f32 = np.float32


def emu_step(case, plant=None):
    def step(i, used):
        return EM.emu_pass(i, case["depths"], case["colors"], case["cams"], used, disp_thresh=case["disp_thresh"],
                           num_consistent=case["num_consistent"], plant=plant)
    return step


@pytest.mark.parametrize("name", list(FC.BUILDERS))
def test_emulation_inside_every_bound(name):
    case = FC.get(name)
    seen = {}
    new = name in FC.NEW
    bad, stats, und, tup = FB.run_case(case, emu_step(case), name=name,
                                       on_pass=(lambda *a: FC.check_reached(name, *a, seen)) if new else None)
    share = sum(und.values()) / max(tup, 1)
    print(f"\n[fusion-ref cpu] {name}: undecided {und} of {tup} = {share:.2e}; decided sets {sum(s['decided_sets'] for s in stats)} of "
          f"{sum(s['active'] for s in stats)}; emulation worst {max(s['pos_ratio'] for s in stats):.3f} of the bound; worst rel bound "
          f"{max(s['bound_rel'] for s in stats):.2e}")
    assert not bad, "\n".join(bad[:20])
    assert share <= FB.UNDECIDED_CAP, f"{name}: {share:.3%} of the tuples undecided"
    assert max(s["bound_rel"] for s in stats) < 1e-5, "the propagated bound undercuts the flat 1e-5 bar it replaces"
    if new:
        FC.check_reached_end(name, stats, seen)


# plant -> the case that must catch it, and in which counters (emit flags, positions, colours, stray marks, missing marks)
PLANT_CASES = {
    "half_even": ("exact_half", ("n_pos", "n_missing", "n_stray")),
    "trunc": ("exact_half", ("n_emit", "n_pos", "n_stray")),
    "disp_le": ("exact_thresh", ("n_pos", "n_stray")),
    "valid_ge": ("nonfinite_thresholds", ("n_emit",)),
    "f_j": ("n4_rolled_ragged", ("n_emit", "n_pos")),
    "t_baseline": ("n4_rolled_ragged", ("n_pos", "n_stray")),
    "no_front": ("behind_loose", ("n_emit", "n_stray")),
    "unrounded_neighbour": ("n3/p1", ("n_pos",)),
    "div_n": ("n3/p1", ("n_pos", "n_rgb")),
    "colour_trunc": ("n3/p1", ("n_rgb",)),
    "need_gt": ("n3/p1", ("n_emit",)),
    "marks_nonemit": ("n9_ragged_behind/p2", ("n_stray",)),
    "skip_used": ("n3/p1", ("n_emit", "n_missing")),
    "double_thresholds": ("nonfinite_thresholds", ("n_emit",)),
}


def test_every_plant_has_a_case():
    assert set(PLANT_CASES) == set(EM.PLANTS)


@pytest.mark.parametrize("plant", EM.PLANTS)
def test_planted_error_is_caught(plant):
    name, counters = PLANT_CASES[plant]
    case = FC.get(name)
    bad, stats, _, _ = FB.run_case(case, emu_step(case, plant), name=name)
    counts = {k: sum(s[k] for s in stats) for k in ("n_emit", "n_pos", "n_rgb", "n_stray", "n_missing")}
    print(f"\n[fusion-ref cpu] plant {plant} in {name}: {counts}, {sum(s['pos_checked'] for s in stats)} decided points")
    assert bad
    for k in counters:
        assert counts[k] > 0, f"{plant}: no {k} violation in {name}: {counts}"


@pytest.mark.parametrize("kind", ["half", "thresh"])
def test_exact_cases_are_exact(kind):
    """Every step of the kernel's chain is exact on the dyadic cases: the reference's bound is zero at each step, so every decision
    is taken at the threshold itself, and the emulation returns the float64 value bit for bit.  The one-step-nearer depths of
    ``thresh`` are fp32 numbers but 10 / d is not: their disparity carries its rounding and is decided all the same.  The mean
    of three points divides by 3 and rounds once; of one, two or four it is exact."""
    case = FC.exact_case(kind)
    used = [u.copy() for u in case["used0"]]
    for i in range(3):
        ref = FB.ref_pass(i, case["depths"], case["colors"], case["cams"], used[i], case["disp_thresh"], debug=True)
        g = ref["dbg"]
        assert ref["undecided"] == {c: 0 for c in FB.CRITERIA}
        for q in ("a", "b", "z", "uh", "vh", "fb"):
            assert (g[q].e == 0).all(), q
        assert all((x.e == 0).all() for x in g["X"])
        uh = g["uh"].v if i == 0 else g["uh"].v[:1]              # (the outer views are 5 columns apart: whole numbers)
        at4 = (g["z"].v == 4) if i == 0 else (g["z"].v[:1] == 4)  # (a pixel of views 1, 2 left at depth 5 shifts by 2 columns)
        assert (i > 0 or at4.sum() >= 40) and (uh[at4] == np.floor(uh[at4])).all(), "every projection 2.5 columns away lands on a half-integer"
        assert (np.abs(g["fb"].v.reshape(-1)) % 10 == 0).all() and np.isin(g["z"].v, (4.0, 5.0)).all()
        plain = g["c0"]["dj"] != np.nextafter(f32(5), f32(4)).astype(np.float64)
        assert (g["disp"].e[plain] == 0).all() and (g["disp"].e[~plain] > 0).all()
        if kind == "thresh" and i == 0:
            on = g["c0"]["ok"] & (g["c0"]["dj"] == 5.0)
            near = g["c0"]["ok"] & ~plain
            assert on.sum() > 20 and (np.abs(g["disp"].v[on]) == 0.5).all() and g["c0"]["cons_f"][on].all()
            assert near.sum() > 20 and g["c0"]["cons_t"][near].all()
        assert all((x.e[g["certain"] & plain] == 0).all() for x in g["Xj"])
        exact_set = ~(g["certain"] & ~plain).any(axis=0)
        pow2 = exact_set & np.isin(g["n"] + 1, (1, 2, 4))
        assert all((o.e[pow2] == 0).all() for o in g["out"])
        xyz, rgb, pix, after = emu_step(case)(i, used)
        dec = FB.decide(ref, case["num_consistent"])
        bad, st = FB.compare(ref, dec, (xyz, rgb, pix), used, after)
        assert not bad, bad
        zero = ref["bound"].reshape(-1, 3)[pix] == 0             # per component: a bound of zero demands the float64 value itself
        assert zero.sum() >= 8 or len(pix) == 0
        np.testing.assert_array_equal(xyz.astype(np.float64)[zero], ref["xyz"].reshape(-1, 3)[pix][zero])
        used = after


def test_colour_rule_is_exact_for_every_sum_and_count():
    """floorf((float)s / (float)(n + 1) + 0.5f) = floor((2 s + n + 1) / (2 (n + 1))) for all n + 1 <= 64, s <= 255 (n + 1)
    (the argument is in tests/_fusion_bounds.py); truncation and round-half-even are not the rule."""
    trunc = even = 0
    for n1 in range(1, 65):
        s = np.arange(255 * n1 + 1)
        assert (s.astype(f32).astype(np.int64) == s).all()
        q = s.astype(f32) / f32(n1)
        want = (2 * s + n1) // (2 * n1)
        np.testing.assert_array_equal(np.floor(q + f32(0.5)).astype(np.int64), want)
        half = (2 * s) % (2 * n1) == n1
        assert (q[half].astype(np.float64) * 2 % 2 == 1).all(), "a half-integer quotient is an fp32 number"
        away = np.abs((s / n1 + 0.5) - np.rint(s / n1 + 0.5))[~half]
        assert away.size == 0 or away.min() >= 1 / (2 * n1) - 1e-12
        trunc += int((np.floor(q).astype(np.int64) != want).sum())
        even += int((np.rint(q).astype(np.int64) != want).sum())
    assert trunc > 0 and even > 0


def test_thresholds_are_fp32_numbers():
    """The kernel holds depth_min, depth_max and disp_thresh as floats: a depth equal to float32(1e-3) is invalid although it exceeds
    the double 1e-3, and the plain rule of tests/_fusion_ref.py says the same."""
    lo, hi = f32(1e-3), f32(1e5)
    assert float(lo) > 1e-3
    d = np.array([lo, np.nextafter(lo, f32(1)), hi, np.nextafter(hi, f32(0)), np.nan, np.inf, -np.inf, 0.0, -1.0], dtype=f32).astype(np.float64)
    np.testing.assert_array_equal(FR.valid(d, 1e-3, 1e5), [False, True, False, True, False, False, False, False, False])
    assert FB.thresholds(0.1)[0] == float(f32(0.1)) != 0.1
    case = FC.get("nonfinite_thresholds")
    with np.errstate(all="ignore"):
        want = FR.fuse_pass(0, case["depths"], case["colors"], case["cams"], case["used0"], disp_thresh=0.5, num_consistent=0)
    got = emu_step(case)(0, case["used0"])
    np.testing.assert_array_equal(np.flatnonzero(want["emit"].reshape(-1)), got[2])


def test_packed_colours_carry_the_top_byte():
    case = FC.get("bytes")
    for p, c, a in zip(FC.packed_colors(case), case["colors"], case["alpha"]):
        u = p.view(np.uint32)
        assert ((u >> 24) == a).all() and a.min() >= 1
        assert ((u & 0xff) == c[..., 0]).all() and (((u >> 8) & 0xff) == c[..., 1]).all() and (((u >> 16) & 0xff) == c[..., 2]).all()
