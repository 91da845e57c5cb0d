"""The cases of the depth-map fusion's reference tests (tests/test_fusion_ref_cpu.py on the CPU, tests/test_gpu_fusion_ref.py and
tests/test_gpu_fusion.py on the GPU), built without a GPU.  A case is a dict: ``depths`` N x float32 [h_v,w_v], ``colors`` N x uint8
[h_v,w_v,3], ``alpha`` None or N x uint8 [h_v,w_v] (the top byte of the packed colour the kernel is handed), ``cams`` float32 [N,30]
(the values of ``ops.geo_filter_cams``), ``used0`` the masks before pass 0, ``disp_thresh``, ``num_consistent``."""
import functools

import numpy as np
import torch

f32 = np.float32


def cam_blocks(K, R, t):
    """[V,3,3], [V,3,3], [V,3,1] torch tensors -> float32 [V,30]: what ``ops.geo_filter_cams`` builds (fp32 ``torch.inverse``)"""
    K = K.to(torch.float32)
    return torch.cat((K.reshape(-1, 9), torch.inverse(K).reshape(-1, 9), R.to(torch.float32).reshape(-1, 9),
                      t.to(torch.float32).reshape(-1, 3)), dim=1).contiguous().numpy()


def _case(depths, colors, cams, thr, need, used0=None, alpha=None):
    depths = [np.ascontiguousarray(d, dtype=f32) for d in depths]
    return {"depths": depths, "colors": [np.ascontiguousarray(c, dtype=np.uint8) for c in colors], "alpha": alpha,
            "cams": np.ascontiguousarray(cams, dtype=f32), "disp_thresh": thr, "num_consistent": need,
            "used0": used0 if used0 is not None else [np.zeros(d.shape, np.uint8) for d in depths]}


def _scene(V, H, W, thr, need, *, crops=None, roll=(), **kw):
    """``synthetic.make_fusion_scene``; ``crops`` {view: (y0, y1, x0, x1)} cuts a window out of a view (its principal point moves
    along); ``roll`` turns those cameras half a turn about their optical axes: R' = diag(-1, -1, 1) R, t' likewise, the principal
    point mirrored to (w - 1 - c_x, h - 1 - c_y) and the maps flipped in both axes -- the same camera centre and the same scene,
    but t' is far from -c, so a baseline taken from |t_i - t_j| is wrong."""
    from wild_deep_mvs_amd import synthetic
    sc = synthetic.make_fusion_scene(V, H, W, seed=kw.pop("seed", 1), **kw)
    depths, colors, K = [d.numpy() for d in sc["depths"]], [c.numpy() for c in sc["colors"]], sc["K"].clone()
    flip = torch.tensor([-1.0, -1.0, 1.0]).reshape(3, 1)
    for v in roll:
        h, w = depths[v].shape
        depths[v], colors[v] = depths[v][::-1, ::-1], colors[v][::-1, ::-1]
        K[v, 0, 2], K[v, 1, 2] = (w - 1) - K[v, 0, 2], (h - 1) - K[v, 1, 2]
        sc["R"][v] = flip * sc["R"][v]
        sc["t"][v] = flip * sc["t"][v]
    for v, (y0, y1, x0, x1) in (crops or {}).items():
        depths[v], colors[v] = depths[v][y0:y1, x0:x1], colors[v][y0:y1, x0:x1]
        K[v, 0, 2] -= x0
        K[v, 1, 2] -= y0
    return _case(depths, colors, cam_blocks(K, sc["R"], sc["t"]), thr, need)


SCENES = {  # the four of tests/test_gpu_fusion.py: (V, H, W, scene options)
    "n3": (3, 48, 64, {}),
    "n9_ragged_behind": (9, 48, 64, {"half_res_view": 3, "behind_view": 5}),
    "n33_ragged": (33, 40, 56, {"half_res_view": 2}),
    "n64_behind": (64, 32, 40, {"behind_view": 7, "spacing": 0.5}),
}
PARAMS = {"p1": (0.1, 2), "p2": (0.5, 3)}       # (disp_thresh, num_consistent)
EXISTING = [f"{c}/{p}" for c in SCENES for p in PARAMS]


def _nonfinite():
    """NaN, +-inf, 0 and negative depths in the reference view and the sources; depths on float32(depth_min) / float32(depth_max)
    exactly (invalid) and one ulp inside (valid).  num_consistent = 0: every valid pixel emits, so validity itself shows."""
    c = _scene(3, 24, 40, 0.5, 0)
    lo, hi = f32(1e-3), f32(1e5)
    vals = [np.nan, np.inf, -np.inf, 0.0, -4.0, lo, hi, np.nextafter(lo, f32(1)), np.nextafter(hi, f32(0)),
            np.nextafter(lo, f32(0)), np.nextafter(hi, f32(np.inf))]
    for v in range(3):
        for k, val in enumerate(vals):
            c["depths"][v][3 + v, 2 + 3 * k] = val
            c["depths"][v][12 + 2 * v, 3 + 3 * k] = val
    return c


def _bytes():
    """used_0 holding 2, 255 and 1 at some pixels (all mean used) and packed colours with a non-zero top byte"""
    c = _scene(3, 24, 40, 0.5, 2)
    rng = np.random.default_rng(11)
    u = c["used0"][0]
    u[2:5, 3:30] = 2
    u[10, :] = 255
    u[15:18, 33:] = 1
    c["used0"][1][6:9, 5:20] = 200          # read by nobody in pass 0 or 2, and by pass 1 as used
    c["alpha"] = [rng.integers(1, 256, d.shape).astype(np.uint8) for d in c["depths"]]
    return c


def exact_case(kind):
    """Hand-built, every quantity a dyadic rational: identity rotations, f = 64, principal point (16, 4), centres 0, +0.15625 and
    -0.15625 along x, reference depth 4, views of 8 x 40.  f B = 10 and the column shift is exactly 2.5 (5 between the outer views):
    seen from view 0, view 1 lands on x - 2.5 (x = 2 on -0.5: target 0, inside) and view 2 on x + 2.5; floor(u + 0.5) rounds both up.
    ``half``: every depth 4.  ``thresh``: disp_thresh = 0.5 and columns of views 1 and 2 at depth 5 (|10 / 4 - 10 / 5| = 0.5 exactly:
    not consistent) or one fp32 step below 5 (consistent)."""
    h, w, f, B = 8, 40, 64.0, 0.15625
    cams = np.zeros((3, 30), dtype=f32)
    for v, cx in enumerate((0.0, B, -B)):
        cams[v, 0:9] = (f, 0, 16, 0, f, 4, 0, 0, 1)
        cams[v, 9:18] = (1 / f, 0, -16 / f, 0, 1 / f, -4 / f, 0, 0, 1)
        cams[v, 18:27] = np.eye(3).reshape(-1)
        cams[v, 27:30] = (-cx, 0, 0)
    depths = [np.full((h, w), 4.0, dtype=f32) for _ in range(3)]
    if kind == "thresh":
        for v in (1, 2):
            depths[v][:, 4::6] = 5.0
            depths[v][:, 7::6] = np.nextafter(f32(5), f32(4))
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    colors = [np.stack(((37 * xs + 11 * ys + 50 * v) % 256, (91 * xs + 3 * ys) % 256, (5 * xs + 77 * ys + 9 * v) % 256), axis=-1)
              for v in range(3)]
    return _case(depths, colors, cams, 0.5, 1 if kind == "thresh" else 2)


def _one_row():
    return _scene(3, 9, 300, 0.1, 2, spacing=0.05, crops={0: (4, 5, 0, 300)})


def _tiny_views():
    return _scene(5, 48, 64, 0.5, 2, crops={1: (20, 25, 30, 37), 3: (24, 25, 32, 33)})


BUILDERS = {
    **{f"{c}/{p}": (lambda c=c, p=p: _scene(*SCENES[c][:3], PARAMS[p][0], min(PARAMS[p][1], SCENES[c][0] - 1), **SCENES[c][3]))
       for c in SCENES for p in PARAMS},
    "n2_37x53": lambda: _scene(2, 37, 53, 0.5, 1),
    "one_row_1x300": _one_row,
    "narrow_5x7_and_1x1": _tiny_views,
    "n64_close": lambda: _scene(64, 24, 40, 0.5, 3, spacing=0.05),
    "segments_130x264": lambda: _scene(3, 130, 264, 0.1, 2),
    "nc0": lambda: _scene(3, 48, 64, 0.1, 0),
    "ncN-1": lambda: _scene(4, 24, 40, 0.5, 3),
    "ncN": lambda: _scene(3, 24, 40, 0.5, 3),
    "behind_loose": lambda: _scene(3, 24, 40, 20.0, 1, behind_view=1),
    "n4_rolled_ragged": lambda: _scene(4, 24, 40, 0.008, 1, half_res_view=2, roll=(3,)),
    "nonfinite_thresholds": _nonfinite,
    "bytes": _bytes,
    "exact_half": lambda: exact_case("half"),
    "exact_thresh": lambda: exact_case("thresh"),
}
NEW = [k for k in BUILDERS if k not in EXISTING]


@functools.lru_cache(maxsize=None)
def get(name):
    return BUILDERS[name]()


def packed_colors(case):
    """int32 [h,w] per view, bytes R, G, B and ``alpha`` (0 without): what ``ops.pack_rgba8`` builds, plus the top byte"""
    out = []
    for v, c in enumerate(case["colors"]):
        a = case["alpha"][v] if case["alpha"] is not None else np.zeros(c.shape[:2], np.uint8)
        out.append(np.ascontiguousarray(np.concatenate((c, a[..., None]), axis=2)).view(np.int32).reshape(c.shape[:2]))
    return out


# ---- what each new case is there to reach: asserted on the reference's own maps and on the outputs, on the CPU and on the GPU ----
def _emitted(ref, got):
    e = np.zeros(ref["active"].size, dtype=bool)
    e[np.asarray(got[2], dtype=np.int64)] = True
    return e.reshape(ref["active"].shape)


def check_reached(name, i, ref, dec, got, before, after, seen):
    """called after pass i of case ``name`` (tests/_fusion_bounds.py::run_case); ``seen`` collects what ``check_reached_end`` asks for"""
    case = get(name)
    emit = _emitted(ref, got)
    h, w = ref["active"].shape
    if name == "one_row_1x300" and i == 0:
        assert (h, w) == (1, 300) and emit.sum() > 50
    elif name == "narrow_5x7_and_1x1":
        if i == 0:
            assert dec["must"][1].sum() > 10 and dec["must"][3].all() and np.asarray(after[3]).all(), "the 5x7 and 1x1 views are consumed"
        if i == 1:
            assert (h, w) == (5, 7)
        if i == 3:
            assert (h, w) == (1, 1)
    elif name == "n64_close" and i == 0:
        assert ref["js"][-1] == 63
        assert (dec["emit_t"] & ref["certain"][-1]).sum() > 100, "view 63 is decidedly consistent with view 0 (bit 63 of hit)"
        assert (np.asarray(after[63]) != 0).sum() > 100
    elif name == "segments_130x264":
        nsx = (w + 31) // 32
        assert h * nsx > 1024
        ys, xs = np.divmod(np.asarray(got[2], dtype=np.int64), w)
        seg = lambda m: np.bincount((np.nonzero(m)[0] * nsx + np.nonzero(m)[1] // 32), minlength=h * nsx)
        cnt = np.bincount(ys * nsx + xs // 32, minlength=h * nsx)
        assert (cnt >= seg(dec["emit_t"])).all() and (cnt <= seg(~dec["emit_f"])).all(), "a segment's count leaves the rule's range"
        seen["irregular"] = max(seen.get("irregular", 0), len(np.unique(cnt)))
    elif name == "nc0":
        lone = dec["emit_t"] & (ref["n_hi"] == 0)
        assert (emit & lone).sum() == lone.sum()
        seen["lone"] = seen.get("lone", 0) + int(lone.sum())
    elif name == "ncN":
        assert len(got[2]) == 0 and all(np.array_equal(a, b) for a, b in zip(after, before)), "num_consistent = N emits and marks nothing"
    elif name == "nonfinite_thresholds":
        for y in (3 + i, 12 + 2 * i):
            off = 2 if y == 3 + i else 3
            cols = off + 3 * np.arange(11)
            assert not ref["active"][y, cols[[0, 1, 2, 3, 4, 5, 6, 9, 10]]].any(), "NaN, inf, <= 0, on or outside a threshold: invalid"
            inside = (np.asarray(before[i])[y, cols[[7, 8]]] == 0)
            assert (ref["active"][y, cols[[7, 8]]] == inside).all() and (emit[y, cols[[7, 8]]] == inside).all(), "one ulp inside: valid"
            seen["inside"] = seen.get("inside", 0) + int(inside.sum())
    elif name == "bytes" and i < 2:
        u = case["used0"][i] != 0
        assert u.sum() > 40 and not ref["active"][u].any() and not emit[u].any(), "a used byte of 2, 200 or 255 means used"
    elif name in ("exact_half", "exact_thresh") and i == 0:
        assert ref["undecided"] == {c: 0 for c in ref["undecided"]}
        xs = np.arange(w)
        c0 = ref["cands"][0]
        for k, shift in ((0, -2), (1, 3)):                      # view 1: x - 2.5 -> x - 2; view 2: x + 2.5 -> x + 3
            inside = (xs + shift >= 0) & (xs + shift < w)
            assert (c0["qx"][k][:, inside] == (xs + shift)[inside]).all() and (c0["qy"][k][:, inside] == np.arange(h)[:, None]).all()
        if name == "exact_half":
            assert (ref["n_lo"] == ((xs >= 2).astype(int) + (xs < w - 3))[None]).all()
            assert (emit == ((xs >= 2) & (xs < w - 3))[None]).all()
            m1, m2 = np.zeros((h, w), np.uint8), np.zeros((h, w), np.uint8)
            m1[:, 0:w - 5], m2[:, 5:w] = 1, 1
            assert np.array_equal(after[1], m1) and np.array_equal(after[2], m2)
        else:
            d1 = case["depths"][1][0]
            on, near = d1 == 5.0, d1 == np.nextafter(f32(5), f32(4))
            tx = xs - 2
            ok = tx >= 0
            cons = ref["certain"][0][0]
            assert on.sum() >= 5 and near.sum() >= 5
            assert not cons[ok][on[tx[ok]]].any(), "|10 / 4 - 10 / 5| = 0.5 = disp_thresh: not consistent"
            assert cons[ok][near[tx[ok]]].all(), "one fp32 step nearer: consistent"
            assert not np.asarray(after[1])[:, on].any() and np.asarray(after[1])[:, near[: w - 2].nonzero()[0]].all()


def check_reached_end(name, stats, seen):
    points = sum(s["points"] for s in stats)
    if name == "ncN":
        assert points == 0
    else:
        assert points > 100 and sum(s["pos_checked"] for s in stats) > 100
    if name == "segments_130x264":
        assert seen["irregular"] >= 8, "segment counts are irregular"
    if name == "nc0":
        assert seen["lone"] > 50, "pixels with no consistent view emit their own unprojection"
    if name == "nonfinite_thresholds":
        assert seen["inside"] >= 4
