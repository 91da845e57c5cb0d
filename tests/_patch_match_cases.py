"""The cases of the PatchMatch reference tests, shared by the CPU file (emulation) and the GPU file (kernel): every shape, source
count, window and top_k of the list, built from synthetic.make_patch_match_scene and hand-built states; all numpy, fp32 inputs."""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np
import torch

from tests import _patch_match_ref as PR

f = np.float32


def _look(c, target):
    z = np.asarray(target, float) - c
    z /= np.linalg.norm(z)
    x = np.cross([0.0, 1.0, 0.0], z)
    x /= np.linalg.norm(x)
    R = np.stack([x, np.cross(z, x), z])
    return R, -R @ c


def _cams(K, R, t):
    from wild_deep_mvs_amd import ops
    return ops.geo_filter_cams(torch.as_tensor(np.stack(K)).float(), torch.as_tensor(np.stack(R)).float(),
                               torch.as_tensor(np.stack(t)).float().reshape(-1, 3, 1)).numpy()


def _scene(V, H, W, seed):
    from wild_deep_mvs_amd import synthetic
    sc = synthetic.make_patch_match_scene(V, H, W, seed=seed)
    greys = [PR.grey(sc["imgs"][v].numpy()) for v in range(V)]
    return sc, greys


def cone_normals(rng, ray, lo_cos, hi_cos):
    """Unit normals facing the camera whose |cos| of the angle to the viewing ray is uniform in [lo_cos, hi_cos]."""
    r = ray / np.linalg.norm(ray, axis=1, keepdims=True)
    a = rng.standard_normal(r.shape)
    a -= (a * r).sum(1, keepdims=True) * r
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    c = rng.uniform(lo_cos, hi_cos, len(r))[:, None]
    return -c * r + np.sqrt(1.0 - c * c) * a


def random_state(rng, h, w, Kinv, dmin, dmax, lo_cos=np.cos(np.radians(75.0)), hi_cos=1.0):
    rows, cols = np.divmod(np.arange(h * w), w)
    ray = np.stack([cols, rows, np.ones(h * w)], -1) @ np.asarray(Kinv, float).T
    n = cone_normals(rng, ray, lo_cos, hi_cos)
    d = 1.0 / rng.uniform(1.0 / dmax, 1.0 / dmin, h * w)
    return np.concatenate([d[:, None], n], 1).reshape(h, w, 4).astype(f)


def _gt_state(sc, v=0):
    return np.concatenate([sc["depth"][v].numpy()[..., None], sc["normal"][v].numpy()], -1).astype(f)


def _case(**kw):
    c = SimpleNamespace(**kw)
    c.h, c.w = c.ref.shape
    c.S = len(c.srcs)
    c.rows, c.cols = np.divmod(np.arange(c.h * c.w), c.w)
    return c


def _plain(name, V, H, W, seed, S, radius, step, top_k, rng_seed, crop_row=None):
    """Reference view 0 and its S nearest views; ``crop_row``: the reference is that single row (its principal point moves up), the
    sources keep their size."""
    sc, greys = _scene(V, H, W, seed)
    src = sc["src"][0][:S]
    K = [sc["K"][i].double().numpy().copy() for i in [0] + src]
    ref, gt = greys[0], _gt_state(sc)
    if crop_row is not None:
        K[0][1, 2] -= crop_row
        ref, gt = np.ascontiguousarray(ref[crop_row: crop_row + 1]), np.ascontiguousarray(gt[crop_row: crop_row + 1])
    cams = _cams(K, [sc["R"][i].numpy() for i in [0] + src], [sc["t"][i].numpy() for i in [0] + src])
    dmin, dmax = float(sc["depth_min"][0]), float(sc["depth_max"][0])
    h, w = ref.shape
    state = random_state(np.random.default_rng(rng_seed), h, w, np.linalg.inv(K[0]), dmin, dmax)
    state[:, : w // 2] = gt[:, : w // 2]
    return _case(name=name, ref=ref, srcs=[greys[s] for s in src], cams=cams, dmin=dmin, dmax=dmax, state=state, gt=gt,
                 sdepths=[(sc["depth"][s].numpy() * f(1.003)).astype(f) for s in src], radius=radius, step=step, top_k=top_k)


def _with_invalid_sources(name, H, W, seed, lowvar):
    """Two scene sources, one looking away (behind), one with a baseline under 1 deg, one turned so part of the view is outside."""
    sc, greys = _scene(3, H, W, seed)
    ref = greys[0].copy()
    if lowvar:
        ref[4:20, 4:20] = 0.5
    K0, R0, t0 = sc["K"][0].double().numpy(), sc["R"][0].double().numpy(), sc["t"][0].double().numpy()
    c0 = -R0.T @ t0[:, 0]
    K, R, t = [sc["K"][i].numpy() for i in range(3)], [sc["R"][i].numpy() for i in range(3)], [sc["t"][i].numpy() for i in range(3)]
    imgs, deps = [greys[1], greys[2]], [sc["depth"][1].numpy(), sc["depth"][2].numpy()]
    extra = [(c0 - 0.5 * R0[2], c0 - 10.0 * R0[2]), (c0 + np.array([0.004, 0.0, 0.0]), c0 + R0[2] * 4.5),
             (c0 + np.array([0.3, 0.0, 0.0]), c0 + R0[2] * 4.5 + np.array([2.5, 0.0, 0.0]))]
    for k, (c, tgt) in enumerate(extra):
        Rk, tk = _look(c, tgt)
        K.append(sc["K"][0].numpy()); R.append(Rk); t.append(tk.reshape(3, 1))
        imgs.append(greys[1 + k % 2]); deps.append(sc["depth"][1 + k % 2].numpy())
    dmin, dmax = float(sc["depth_min"][0]), float(sc["depth_max"][0])
    gt = _gt_state(sc)
    state = random_state(np.random.default_rng(3), H, W, np.linalg.inv(K0), dmin, dmax)
    state[:, : W // 2] = gt[:, : W // 2]
    return _case(name=name, ref=ref, srcs=imgs, cams=_cams(K, R, t), dmin=dmin, dmax=dmax, state=state, gt=gt,
                 sdepths=[(d * f(1.003)).astype(f) for d in deps], radius=5, step=1, top_k=3)


EDGE_HYPOTHESES = {"d=0": (0.0, None), "d<0": (-3.0, None), "d=nan": (np.nan, None), "d=inf": (np.inf, None),
                   "n=0": (None, (0.0, 0.0, 0.0)), "n away": (None, "flip")}


def _exact_with_edges():
    c = _plain("exact16x32+edges", 5, 16, 32, 4, 4, 8, 1, 4, 11)
    c.edge_pixels = {}
    for i, (key, (d, n)) in enumerate(EDGE_HYPOTHESES.items()):
        r, col = 8, 18 + 2 * i                       # every second pixel: each item has ordinary neighbours
        if d is not None:
            c.state[r, col, 0] = d
        if n == "flip":
            c.state[r, col, 1:] = -c.state[r, col, 1:]
        elif n is not None:
            c.state[r, col, 1:] = n
        c.edge_pixels[key] = (r, col)
    return c


def _mixed_res():
    """A half-resolution source with its own intrinsics, a 2 x 2 source and a full-size one."""
    sc, greys = _scene(4, 16, 32, 6)
    H, W = 16, 32
    half = np.array([[0.5, 0.0, -0.25], [0.0, 0.5, -0.25], [0.0, 0.0, 1.0]])
    g1 = greys[1].reshape(H // 2, 2, W // 2, 2).mean((1, 3)).astype(f)
    d1 = sc["depth"][1].numpy().reshape(H // 2, 2, W // 2, 2).mean((1, 3)).astype(f)
    tiny = np.array([[2.0 / W, 0.0, 0.5 / W * 2 - 0.5], [0.0, 2.0 / H, 0.5 / H * 2 - 0.5], [0.0, 0.0, 1.0]])
    g2 = greys[2].reshape(2, H // 2, 2, W // 2).mean((1, 3)).astype(f)
    d2 = sc["depth"][2].numpy().reshape(2, H // 2, 2, W // 2).mean((1, 3)).astype(f)
    K = [sc["K"][0].numpy(), half @ sc["K"][1].double().numpy(), tiny @ sc["K"][2].double().numpy(), sc["K"][3].numpy()]
    cams = _cams(K, [sc["R"][i].numpy() for i in range(4)], [sc["t"][i].numpy() for i in range(4)])
    dmin, dmax = float(sc["depth_min"][0]), float(sc["depth_max"][0])
    gt = _gt_state(sc)
    state = random_state(np.random.default_rng(8), H, W, np.linalg.inv(sc["K"][0].double().numpy()), dmin, dmax)
    state[:, : W // 2] = gt[:, : W // 2]
    return _case(name="mixed-res16x32", ref=greys[0], srcs=[g1, g2, greys[3]], cams=cams, dmin=dmin, dmax=dmax, state=state, gt=gt,
                 sdepths=[d1, d2, (sc["depth"][3].numpy() * f(1.003)).astype(f)], radius=1, step=1, top_k=1)


def _grazing():
    c = _plain("grazing16x32", 3, 16, 32, 7, 2, 5, 1, 2, 12)
    c.state = random_state(np.random.default_rng(13), c.h, c.w, np.linalg.inv(c.cams[0, 0:9].reshape(3, 3).astype(float)), c.dmin,
                           c.dmax, 0.01, 0.1)
    return c


def _dyadic():
    """Every step of both projections is exact in fp32: K = (64, 64, 16, 8), R = I, t = (3/32, 0, 0), the fronto-parallel plane
    d = 4 at every pixel -> the source column is col + 1.5, decidedly a half-integer; the source's depth 3 brings the half-away
    rounding back onto the pixel (e_s = 0) and a half-even one a pixel off (e_s = 1).  The propagated planes are bit-identical to
    the current one (ties), the triangulation angle is 1.34 deg (between the 1 deg and the 3 deg tests)."""
    H, W = 8, 16
    K = np.array([[64.0, 0.0, 16.0], [0.0, 64.0, 8.0], [0.0, 0.0, 1.0]])
    cams = _cams([K, K], [np.eye(3), np.eye(3)], [np.zeros((3, 1)), np.array([[3.0 / 32], [0.0], [0.0]])])
    tex = lambda x, y: 0.5 + 0.25 * np.sin(0.9 * x + 0.4 * y) + 0.15 * np.cos(0.5 * x - 1.1 * y)
    ys, xs = np.meshgrid(np.arange(H, dtype=float), np.arange(W + 4, dtype=float), indexing="ij")
    ref, src = tex(xs[:, :W], ys[:, :W]).astype(f), tex(xs - 1.5, ys).astype(f)
    state = np.zeros((H, W, 4), f)
    state[..., 0], state[..., 3] = 4.0, -1.0
    return _case(name="dyadic8x16", ref=ref, srcs=[src], cams=cams, dmin=2.0, dmax=8.0, state=state, gt=state.copy(),
                 sdepths=[np.full((H, W + 4), 3.0, f)], radius=1, step=1, top_k=1)


def _rm_edge():
    """The dyadic camera moved 24 along the axis: the plane d = 4 maps column col to (col + 96) / 7 exactly, so column 2 lands on
    the source's last column 14 = w_s - 1, decidedly inside, and the correctly rounded quotient says so; 98 * fl(1 / 7) rounds
    to the next fp32 number above 14, outside.  Columns 0 and 1 are inside, columns 3.. decidedly outside."""
    H, W = 8, 16
    K = np.array([[64.0, 0.0, 16.0], [0.0, 64.0, 8.0], [0.0, 0.0, 1.0]])
    cams = _cams([K, K], [np.eye(3), np.eye(3)], [np.zeros((3, 1)), np.array([[0.0], [0.0], [24.0]])])
    rng = np.random.default_rng(21)
    ref, src = rng.uniform(0.2, 0.8, (H, W)).astype(f), rng.uniform(0.2, 0.8, (9, 15)).astype(f)
    state = np.zeros((H, W, 4), f)
    state[..., 0], state[..., 3] = 4.0, -1.0
    return _case(name="rm-edge8x16", ref=ref, srcs=[src], cams=cams, dmin=2.0, dmax=8.0, state=state, gt=state.copy(),
                 sdepths=[np.full((9, 15), 28.0, f)], radius=1, step=1, top_k=1)


BUILDERS = {
    "ragged17x33": lambda: _with_invalid_sources("ragged17x33", 17, 33, 1, False),
    "exact16x32+edges": _exact_with_edges,
    "existing40x56": lambda: _with_invalid_sources("existing40x56", 40, 56, 0, True),
    "tiny5x7": lambda: _plain("tiny5x7", 3, 5, 7, 2, 1, 5, 1, 1, 9),
    "row1x40": lambda: _plain("row1x40", 4, 9, 40, 3, 2, 8, 2, 2, 10, crop_row=4),
    "maxsrc17x33": lambda: _plain("maxsrc17x33", 32, 17, 33, 5, 31, 4, 4, 8, 14),
    "mixed-res16x32": _mixed_res,
    "dyadic8x16": _dyadic,
    "rm-edge8x16": _rm_edge,
    "grazing16x32": _grazing,
}
COST_CASES = [k for k in BUILDERS if k != "grazing16x32"]
# (case, geometric, colour, converged)
HALF_CASES = [("ragged17x33", g, c, conv) for g in (False, True) for c in (0, 1) for conv in (False, True)] + \
    [(k, False, 0, False) for k in ("exact16x32+edges", "tiny5x7", "row1x40", "maxsrc17x33", "mixed-res16x32")] + \
    [(k, True, 1, True) for k in ("exact16x32+edges", "tiny5x7", "row1x40", "maxsrc17x33", "mixed-res16x32")] + \
    [("dyadic8x16", False, 0, True)]
FILTER_CASES = ["ragged17x33", "exact16x32+edges", "tiny5x7", "row1x40", "maxsrc17x33", "mixed-res16x32", "dyadic8x16"]
HALF_SEED, HALF_VIEW, HALF_T = 5, 7, 2


@functools.lru_cache(maxsize=None)
def case(name):
    return BUILDERS[name]()


def half_state(c, converged):
    return c.gt.copy() if converged else c.state.copy()


@functools.lru_cache(maxsize=None)
def cost_models(name):
    """(cost model, e_s model) of the case's state at every pixel: computed once, shared, never modified."""
    from tests import _patch_match_bounds as PB
    c = case(name)
    st = c.state.reshape(-1, 4)
    return (PB.cost_model(c.ref, c.srcs, c.cams, c.rows, c.cols, st[:, 0], st[:, 1:], c.radius, c.step),
            PB.geom_model(c.cams, c.sdepths, c.rows, c.cols, st[:, 0]))


@functools.lru_cache(maxsize=None)
def filter_models(name):
    from tests import _patch_match_bounds as PB
    c = case(name)
    return PB.filter_model(c.state, c.ref, c.srcs, c.cams, c.sdepths, c.radius, c.step)


def half_args(c, geometric, colour):
    from tests import _patch_match_ref as PR
    delta, theta = PR.schedule(HALF_T)
    return dict(colour=colour, iteration=(int(geometric) << 16) | HALF_T, delta=delta, theta=theta, seed=HALF_SEED, view=HALF_VIEW)


def agg_of(c, geometric, colour):
    """The float64 aggregated cost and its bound of given fp32 hypotheses at pixels of the colour (for check_choice)."""
    from tests import _patch_match_bounds as PB
    rows, cols = PR.colour_pixels(c.h, c.w, colour)
    win = PB.window_model(c.ref, rows, cols, c.radius, c.step)

    def fn(k, idx, hyp):
        w_k = {key: (val[idx] if key not in ("oy", "ox") else val) for key, val in win.items()}
        cm = PB.cost_model(c.ref, c.srcs, c.cams, rows[idx], cols[idx], hyp[:, 0], hyp[:, 1:], c.radius, c.step, window=w_k)
        gm = PB.geom_model(c.cams, c.sdepths, rows[idx], cols[idx], hyp[:, 0]) if geometric else None
        agg, ab, _ = PB.aggregate_model(cm, gm, c.top_k)
        return agg, ab
    return fn


# ---------------------------------------------------------------------------------------------------------------------------
# verification drivers: the same checks for the emulation (CPU) and the kernel (GPU)
# ---------------------------------------------------------------------------------------------------------------------------
def verify_cost(name, geometric, got_c, got_e, got_agg):
    """-> (results of PB.check_cost, {share name: value})."""
    from tests import _patch_match_bounds as PB
    c = case(name)
    cm, gm = cost_models(name)
    res = PB.check_cost(cm, gm if geometric else None, c.top_k, np.asarray(got_c).reshape(c.S, -1),
                        None if got_e is None else np.asarray(got_e).reshape(c.S, -1), np.asarray(got_agg).reshape(-1))
    both = cm["valid"] & cm["vdec"]
    shares = dict(undecided=PB.undecided_share(cm), e_undecided=float((~gm["rdec"]).mean()),
                  vacuous=float((cm["cb"][both] * PB.SCALE["cost"] > 1e-3).mean()) if both.any() else 0.0,
                  valid=float(cm["valid"].mean()), bound_max=float(cm["cb"][both].max()) if both.any() else 0.0)
    return res, shares


@functools.lru_cache(maxsize=None)
def candidate_models(name, geometric, colour, converged):
    from tests import _patch_match_bounds as PB
    c = case(name)
    rows, cols = PR.colour_pixels(c.h, c.w, colour)
    return PB.candidate_model(half_state(c, converged), c.cams, rows, cols, c.dmin, c.dmax, **half_args(c, geometric, colour))


def verify_half(name, geometric, colour, converged, new_state, choice, cand):
    """new_state [h,w,4], choice [h,w], cand [h,w,11,4] as the half-step left them -> (results, info)."""
    from tests import _patch_match_bounds as PB
    c = case(name)
    st0 = half_state(c, converged)
    mine = ((np.add.outer(np.arange(c.h), np.arange(c.w)) & 1) == colour)
    new_state, choice, cand = np.asarray(new_state, dtype=f), np.asarray(choice), np.asarray(cand, dtype=f)
    cdm = candidate_models(name, geometric, colour, converged)
    res = PB.check_candidates(cdm, cand[mine])
    bits = lambda a: np.ascontiguousarray(a, dtype=f).view(np.uint32)
    res["other_colour"] = (int((bits(new_state[~mine]) != bits(st0[~mine])).sum()) + int((choice[~mine] != -1).sum()), int((~mine).sum()), 0.0)
    ch = choice[mine].astype(np.int64)
    pick = cand[mine][np.arange(len(ch)), np.clip(ch, 0, 10)]
    res["written"] = (int((bits(new_state[mine]) != bits(pick)).any(-1).sum()), len(ch), 0.0)
    r2, sure = PB.check_choice(cand[mine], ch, agg_of(c, geometric, colour))
    res.update(r2)
    und = 1.0 - float(cdm["ldec"][1:9].mean())
    return res, dict(index_checked=sure, live_undecided=und, branch_undecided=1.0 - float(cdm["cdec"][9:].mean()))


def verify_filter(name, got_depth, got_normal, got_count):
    from tests import _patch_match_bounds as PB
    c = case(name)
    fm = filter_models(name)
    res = PB.check_filter(fm, c.state, got_depth, got_normal, got_count)
    und = sum(int((~fm["passes"][k][1]).sum()) for k in PB.FILTER_CRITERIA) / (3 * fm["ok"].size)
    return res, dict(filter_undecided=und, all_decided=float(fm["okdec"].all(0).mean()), kept=float((np.asarray(got_count) >= 2).mean()))
