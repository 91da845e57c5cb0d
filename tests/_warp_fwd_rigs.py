"""Hand-written camera rigs of tests/test_gpu_warp_fwd.py, kept apart from it so that tests/test_warp_fwd_ref_cpu.py can check every
one of them WITHOUT a GPU: the fragile share (tests/_warp_bwd_ref.py ``fragile``) stays below the cap, the cameras are partly behind
where a case says so, and the staging mode a case of group B names is the one the box rule of csrc/warp_box.h gives (restated here on
float64 corner projections: ``staging_modes``).

A rig is a dict: cams [n,B,18] fp32 (passed to ``ops.warp_cost`` as they are), depth [B,D] or [B,D,h,w] fp32, geom, ref_hw, src_hw,
ref_y0.  No builder of the package stands between these numbers and the kernel."""
import torch

import _warp_bwd_ref as R

FRAGILE_CAP = 0.005
DIRECT, GEN, FAST, ZERO = 0, 1, 2, 3


def _rig(cams, depth, geom, ref_hw, src_hw, ref_y0=0):
    return {"cams": cams.float().contiguous(), "depth": depth.float().contiguous(), "geom": geom, "ref_hw": tuple(ref_hw),
            "src_hw": tuple(src_hw), "ref_y0": int(ref_y0)}


def fragile_share(rig):
    """Share of voxels with a fragile sample in any view, from the float64 reference alone."""
    f = R.fragile(rig["cams"], rig["depth"], rig["geom"], rig["ref_hw"], rig["src_hw"], rig["ref_y0"])
    return float(f.any(dim=0).double().mean())


def _jitter(depth, ref_hw, seed, amp=0.1):
    """Per-pixel planes: every plane of every item times 1 +- amp / 2, differently at every pixel."""
    B, D = depth.shape
    gen = torch.Generator().manual_seed(seed)
    return (depth.view(B, D, 1, 1) * (1.0 + amp * (torch.rand(B, D, *ref_hw, generator=gen) - 0.5))).contiguous()


# ---- A. mode and type matrix ------------------------------------------------------------------------------------------------------
A_REF, A_SRC, A_D = (11, 21), (23, 29), 6        # ragged 8 x 4 tiles each way; both source extents >= 21 (staged group correlation)


def matrix_rig(geom, per_pixel, seed=0):
    """Two views, two items whose cameras and depth rows DIFFER.  View 0: a mild affine map with a little perspective, wholly in
    front.  View 1: q_z = 1 - 0.2 x + ... crosses zero between two pixel columns (|q_z| >= 0.1 on either side, so that no column is
    ill-conditioned): the columns to its right lie behind that camera, the ones before it sweep through the source map and out of it."""
    cams = torch.zeros(2, 2, 18)
    for b in range(2):
        cams[0, b, :12] = torch.tensor([1.04 + 0.03 * b, 0.03, 0.4, -0.02, 1.02 - 0.02 * b, 0.3 + 0.2 * b, 0.004, -0.003, 1.0,
                                        0.5 - 0.3 * b, -0.4, 0.05 * b])
        if geom == "proj":
            cams[1, b, :12] = torch.tensor([1.1, 0.02, 0.3, -0.03, 1.05, 0.2 + 0.1 * b, -0.21 - 0.01 * b, 0.0, 1.0, 0.3, 0.2 * b, 0.02])
        else:                               # block[9:18] = Bm: hom = A p - (Bm p) / (d + 1e-9), half-pixel centres
            cams[0, b, 9:] = torch.tensor([0.3, 0.0, 0.5 + 0.2 * b, 0.0, 0.2, -0.4, 0.001, 0.0, 0.03])
            cams[1, b, :9] = torch.tensor([1.1, 0.02, 0.3, -0.03, 1.05, 0.2 + 0.1 * b, -0.2 - 0.004 * b, 0.0, 1.0])
            cams[1, b, 9:] = torch.tensor([-0.2, 0.0, 0.4, 0.0, 0.1, 0.3 - 0.2 * b, 0.002, 0.0, -0.01])
    depth = torch.stack([torch.linspace(1.0, 2.0, A_D), torch.linspace(1.3, 2.6, A_D)])
    if per_pixel:
        depth = _jitter(depth, A_REF, 100 + seed)
    rig = _rig(cams, depth, geom, A_REF, A_SRC)
    assert_partly_behind(rig, view=1, front_view=0)
    assert not torch.equal(cams[:, 0], cams[:, 1]) and not torch.equal(depth[0], depth[1])
    return rig


def assert_partly_behind(rig, view, front_view=None):
    """(checked on the CPU: without it a case would silently test something else)"""
    ix, iy, qz = R.positions(rig["cams"], rig["depth"], rig["geom"], rig["ref_hw"], rig["src_hw"], rig["ref_y0"])
    hs, ws = rig["src_hw"]
    for b in range(qz.shape[1]):
        behind = float((qz[view, b] <= 0).double().mean())
        inside = float(((qz[view, b] > 0) & (ix[view, b] > 0) & (ix[view, b] < ws - 1) & (iy[view, b] > 0) & (iy[view, b] < hs - 1)).double().mean())
        assert 0.1 < behind < 0.9 and inside > 0.1, (rig["geom"], b, behind, inside)
        if front_view is not None:
            assert float((qz[front_view, b] > 0).double().mean()) == 1.0


# ---- the box rule of the staged kernels, restated (csrc/warp_box.h, csrc/warp_lds.h: corner projections -> box -> mode -> arena) ----
TILE_W, TILE_H = 8, 4
POLICY = {"quad_owner": dict(pad=0, pitch_round=4, max_w=16, max_h=8, arena=316),
          "lane_owner": dict(pad=2, pitch_round=1, max_w=32, max_h=16, arena=416),
          "groupcorr": dict(pad=2, pitch_round=1, max_w=32, max_h=16, arena=416)}


def planes_per_block(tiles, D, start=32, floor=4, min_blocks=1024, override=0, cap=64):
    """plan_planes of warp_box.h for the staged kernels (even plane counts)."""
    ppd = start
    if override > 0:
        ppd = min((override + 1) & ~1, cap)
    while ppd > floor and tiles * ((D + ppd - 1) // ppd) < min_blocks:
        ppd >>= 1
    return ppd


def staging_modes(rig, kernel, grow=0.0, ppd=None):
    """[n_src,4] counts of (DIRECT, GEN, FAST, ZERO) over the (tile, plane chunk) blocks of a launch WITHOUT the adaptive split, as
    the staged kernel ``kernel`` decides them: the 8 corner projections (tile corners x depth extremes of the chunk) in float64, a
    slack of 1/32 texel (+ ``grow``: a case asserts its mode with the slack a little larger and smaller, so that fp32 rounding of a
    corner cannot change it), floor, the clipped box against the largest box, then the greedy arena.  Per-batch planes only."""
    pol = POLICY[kernel]
    cams, depth, geom = rig["cams"].double(), rig["depth"].double(), rig["geom"]
    (h, w), (hs, ws) = rig["ref_hw"], rig["src_hw"]
    n, B = cams.shape[:2]
    D = depth.shape[1]
    assert depth.dim() == 2 and n <= 4
    nty, ntx = (h + TILE_H - 1) // TILE_H, (w + TILE_W - 1) // TILE_W
    ppd = planes_per_block(B * nty * ntx, D) if ppd is None else ppd
    off = 0.5 if geom == "homog" else 0.0
    sx, sy = ((ws - 1) / ws, (hs - 1) / hs) if geom == "homog" else (1.0, 1.0)
    hist = torch.zeros(n, 4, dtype=torch.int64)
    sl = 1.0 / 32 + grow
    for b in range(B):
        for ty in range(nty):
            for tx in range(ntx):
                xs = (tx * TILE_W + off, min(tx * TILE_W + TILE_W - 1, w - 1) + off)
                ys = (ty * TILE_H + off + rig["ref_y0"], min(ty * TILE_H + TILE_H - 1, h - 1) + off + rig["ref_y0"])
                for d0 in range(0, D, ppd):
                    dd = depth[b, d0:d0 + ppd]
                    used = 0
                    for v in range(n):
                        c = cams[v, b]
                        us, vs, ok = [], [], True
                        for d in (float(dd.min()), float(dd.max())):
                            for cy in ys:
                                for cx in xs:
                                    a3 = [float(c[3 * i] * cx + c[3 * i + 1] * cy + c[3 * i + 2]) for i in range(3)]
                                    if geom == "proj":
                                        q = [a3[i] * d + float(c[9 + i]) for i in range(3)]
                                    else:
                                        q = [a3[i] - float(c[9 + 3 * i] * cx + c[10 + 3 * i] * cy + c[11 + 3 * i]) / (d + 1e-9) for i in range(3)]
                                    if not q[2] > 1e-6:
                                        ok = False
                                        continue
                                    us.append(q[0] / q[2] * sx)
                                    vs.append(q[1] / q[2] * sy)
                        mode, need = DIRECT, 0
                        if ok:
                            fl = lambda t: int(torch.floor(torch.tensor(t, dtype=torch.float64)))
                            X0, X1, Y0, Y1 = fl(min(us) - sl), fl(max(us) + sl) + 1, fl(min(vs) - sl), fl(max(vs) + sl) + 1
                            outside = X1 < 0 or Y1 < 0 or X0 > ws - 1 or Y0 > hs - 1
                            inside = X0 >= 0 and Y0 >= 0 and X1 <= ws - 1 and Y1 <= hs - 1
                            bw = min(X1, ws - 1 + pol["pad"]) - max(X0, -pol["pad"]) + 1
                            bh = min(Y1, hs - 1 + pol["pad"]) - max(Y0, -pol["pad"]) + 1
                            if outside:
                                mode = ZERO
                            elif bw <= pol["max_w"] and bh <= pol["max_h"]:
                                mode = FAST if inside else GEN
                                need = ((bw + pol["pitch_round"] - 1) & ~(pol["pitch_round"] - 1)) * bh
                        if mode in (FAST, GEN):
                            if used + need > pol["arena"]:
                                mode = DIRECT
                            else:
                                used += need
                        hist[v, mode] += 1
    return hist


# ---- B. staging modes -------------------------------------------------------------------------------------------------------------
B_REF, B_D, B_VIEWS = (10, 20), 5, 4
B_SHIFTS = ((0.37, 0.61), (0.71, 0.23), (0.13, 0.47), (0.55, 0.83))
# zoom of the "box too large" and "arena full" cases per kernel: an 8 x 4 tile spreads over about (7 z + 2) x (3 z + 2) texels
B_ZOOM = {"quad_owner": {"too_large": 3.0, "arena_full": 1.7}, "lane_owner": {"too_large": 5.5, "arena_full": 2.5},
          "groupcorr": {"too_large": 5.5, "arena_full": 2.5}}
B_MODES = ("fast", "gen", "zero", "too_large", "arena_full", "behind")


def zoom_rig(kernel, mode):
    """Pure scaling by z about the origin plus a shift, four views, one item.  PROJ: rot = diag(z, z, 1), trans = (tx, ty, 0): pixel x
    on plane d samples z x + tx / d.  HOMOG (the group-correlation kernel): A = the same divided by the index scale (size - 1) / size on
    half-pixel centres, Bm = 0.  ``mode``: fast -- everything inside; gen -- view 1 shifted by -1.3 texels (the boxes of the first tile
    row and column are clipped); zero -- view 2 shifted wholly outside; too_large -- a zoom whose boxes exceed the largest box;
    arena_full -- a zoom at which every box fits the largest box but only the first views fit the arena; behind -- view 3 with
    q_z = 1 - 0.2 x ..., whose tiles all have a corner behind the camera."""
    geom = "homog" if kernel == "groupcorr" else "proj"
    z = B_ZOOM[kernel].get(mode, 1.0)
    hs, ws = max(int(B_REF[0] * z) + 3, 23), max(int(B_REF[1] * z) + 3, 23)
    cams = torch.zeros(B_VIEWS, 1, 18)
    for v, (tx, ty) in enumerate(B_SHIFTS):
        if mode == "gen" and v == 1:
            tx, ty = -1.3, -1.6
        if mode == "zero" and v == 2:
            tx, ty = -200.0, 0.3
        pz = -0.2 if (mode == "behind" and v == 3) else 0.0
        if geom == "proj":
            cams[v, 0, :12] = torch.tensor([z, 0, 0, 0, z, 0, pz * 1.05, 0, 1.0, tx, ty, 0.02 if pz else 0.0])
        else:
            cams[v, 0, :9] = torch.tensor([z * ws / (ws - 1), 0, tx, 0, z * hs / (hs - 1), ty, pz, 0, 1.0])
    return _rig(cams, torch.linspace(1.0, 2.0, B_D).view(1, B_D), geom, B_REF, (hs, ws))


def check_zoom_rig(kernel, mode):
    """The case means what its name says: asserted on the box rule restated above, with the slack 1/64 texel larger and smaller."""
    rig = zoom_rig(kernel, mode)
    hists = [staging_modes(rig, kernel, g) for g in (-1.0 / 64, 0.0, 1.0 / 64)]
    for hm in hists:
        only = lambda v, m: int(hm[v, m]) == int(hm[v].sum()) > 0
        if mode == "fast":
            assert all(only(v, FAST) for v in range(B_VIEWS)), hm
        elif mode == "gen":
            assert int(hm[1, GEN]) > 0 and int(hm[1, DIRECT]) == 0 and all(only(v, FAST) for v in (0, 2, 3)), hm
        elif mode == "zero":
            assert only(2, ZERO) and all(only(v, FAST) for v in (0, 1, 3)), hm
        elif mode == "too_large":
            assert all(int(hm[v, DIRECT]) > 0 for v in range(B_VIEWS)), hm
        elif mode == "arena_full":
            assert int(hm[0, DIRECT]) == 0 and int(hm[B_VIEWS - 1, DIRECT]) > 0, hm
        else:
            assert only(3, DIRECT) and all(only(v, FAST) for v in (0, 1, 2)), hm
    if mode == "arena_full":            # each box alone fits: a launch with any single view stages it everywhere
        for v in range(B_VIEWS):
            one = dict(rig, cams=rig["cams"][v:v + 1])
            assert int(staging_modes(one, kernel)[0, DIRECT]) == 0, v
    return rig, hists[1]


# ---- C. plane ranges --------------------------------------------------------------------------------------------------------------
C_SRC_PAD = 48
# The staged kernels halve their 32 planes per workgroup while a launch has fewer than 1024 workgroups (plan_planes, warp_box.h), so a
# chunk of 12 planes exists at D = 44 only in a launch of at least 512 tiles of 8 x 4 pixels.  128 items of a 5 x 9 reference (one
# full tile and three ragged ones each) are the cheapest such launch: 253 000 voxels.
C_SHAPES = {44: ((5, 9), 128), 5: ((16, 24), 1), 1: ((16, 24), 1)}       # D -> reference size, batch items


def range_rig(D):
    """Pure translation along x that grows with the plane index: rot = (1 0 c; 0 1 0; 0 0 1), trans = (t, ty, 0), planes
    d_k = 1 / (0.1 + 0.01 k), so that pixel x on plane k samples x + c + (t / 100) (10 + k): s = t / 100 texels per plane.
    View 0, s = 0.8: a 12-plane box is 9 + 8.8 texels wide -- too wide for the quad-owner kernel's 16, its 6-plane halves fit.
    View 1, s = 1.5: 6-plane halves are 17-18 wide, the 4- and 2-plane quarters fit.  View 2, s = 3: a 4-plane chunk is 18-19 wide and
    its 2-plane halves fit; 12 planes exceed the lane-owner kernel's 32 as well.  The offsets c keep the early planes of views 1 and 2
    partly left of the map (clipped boxes, boxes outside) and the late planes of view 2 right of it; item b adds 0.37 (b mod 16)."""
    (h, w), B = C_SHAPES[D]
    k = torch.arange(D, dtype=torch.float64)
    depth = (1.0 / (0.1 + 0.01 * k)).view(1, D).repeat(B, 1)
    cams = torch.zeros(3, B, 18)
    offsets = (-13.0, -35.0, -70.0) if D > 8 else (-8.5, -16.0, -29.0)      # (few planes: everything near the left border of the map)
    for v, (per_plane, c) in enumerate(zip((0.8, 1.5, 3.0), offsets)):
        for b in range(B):
            cams[v, b, :12] = torch.tensor([1.0, 0, c + 0.37 * (b % 16), 0, 1.0, 0, 0, 0, 1.0, per_plane * 100.0, 0.4 + 0.1 * v, 0.0])
    return _rig(cams, depth, "proj", (h, w), (h + 3, w + C_SRC_PAD))


# ---- D. host-path edges -----------------------------------------------------------------------------------------------------------
def many_views_rig(n=16):
    """HOMOG, 16 source views (the dynamic-LDS opt-in of the generic kernel), 12 x 16 reference, D = 3: small affine maps that differ
    per view and item, with a plane-dependent part."""
    ref_hw, src_hw, D = (12, 16), (14, 19), 3
    cams = torch.zeros(n, 2, 18)
    for v in range(n):
        for b in range(2):
            s = 1.0 + 0.01 * v - 0.02 * b
            cams[v, b, :9] = torch.tensor([1.15 * s, 0.02 * (v % 3), 0.3 + 0.1 * v, -0.01 * (v % 4), 1.12 * s, 0.2 + 0.05 * v, 0.002 * (v % 5), -0.001 * b, 1.0])
            cams[v, b, 9:] = torch.tensor([0.3 - 0.04 * v, 0.0, 0.4, 0.0, 0.2, -0.3 + 0.03 * v, 0.001, 0.0, 0.02])
    depth = torch.stack([torch.linspace(1.0, 2.0, D), torch.linspace(1.4, 2.2, D)])
    return _rig(cams, depth, "homog", ref_hw, src_hw)


def narrow_source_rig():
    """HOMOG with a 9 x 15 source map: the clamp -0.05 (size - 1) lies inside the border texel, so the rays behind the camera (sent to
    -10, then clamped) carry a non-zero weight.  View 1 crosses q_z = 0 inside the image; item 1 of view 0 has the third rows of A and
    Bm equal to ZERO: q_z == 0 exactly at every sample (not fragile: see ``fragile``), which the kernels must treat as behind."""
    ref_hw, src_hw, D = (11, 21), (9, 15), 4
    cams = torch.zeros(2, 2, 18)
    for b in range(2):
        cams[0, b, :9] = torch.tensor([0.7, 0.02, 0.4, -0.02, 0.75, 0.3 + 0.2 * b, 0.003, -0.002, 1.0])
        cams[0, b, 9:] = torch.tensor([0.3, 0.0, 0.5, 0.0, 0.2, -0.4, 0.001, 0.0, 0.03])
        cams[1, b, :9] = torch.tensor([0.75, 0.02, 0.3, -0.03, 0.7, 0.2 + 0.1 * b, -0.2 - 0.004 * b, 0.0, 1.0])
        cams[1, b, 9:] = torch.tensor([-0.2, 0.0, 0.4, 0.0, 0.1, 0.3 - 0.2 * b, 0.002, 0.0, -0.01])
    cams[0, 1, 6:9] = 0.0
    cams[0, 1, 15:18] = 0.0
    depth = torch.stack([torch.linspace(1.0, 2.0, D), torch.linspace(1.3, 2.6, D)])
    rig = _rig(cams, depth, "homog", ref_hw, src_hw)
    ix, iy, qz = R.positions(rig["cams"], rig["depth"], "homog", ref_hw, src_hw)
    assert bool((qz[0, 1] == 0).all()) and bool((ix[0, 1] == -0.05 * (src_hw[1] - 1)).all())
    assert -0.05 * (src_hw[1] - 1) > -1 and 0 < float((qz[1] <= 0).double().mean()) < 1
    return rig


def sized_source_rig(which):
    """PROJ, three views, a source map smaller (9 x 14) or larger (31 x 40) than the 12 x 20 reference."""
    ref_hw = (12, 20)
    src_hw = {"smaller": (9, 14), "larger": (31, 40)}[which]
    z = src_hw[1] / ref_hw[1]
    cams = torch.zeros(3, 2, 18)
    for v in range(3):
        for b in range(2):
            cams[v, b, :12] = torch.tensor([z * (0.9 + 0.05 * v), 0.02, 0.1, -0.01, z * (0.92 - 0.03 * b), 0.2, 0.003 * v, -0.002, 1.0,
                                            0.6 - 0.5 * v, 0.3 + 0.4 * b, 0.05 * v])
    depth = torch.stack([torch.linspace(1.0, 2.0, 5), torch.linspace(1.2, 2.9, 5)])
    return _rig(cams, depth, "proj", ref_hw, src_hw)


SLAB_ROWS, SLAB_Y0, SLAB_H = 13, 3, 6


def slab_rig(geom, per_pixel, whole=False):
    """Rows [3, 9) of a 13-row grid (``whole``: the grid itself), the matrix rig's cameras with three views' worth of variety."""
    base = matrix_rig(geom, False)
    w = A_REF[1]
    depth = base["depth"]
    full_hw = (SLAB_ROWS, w)
    if per_pixel:
        depth = _jitter(depth, full_hw, 300)
        if not whole:
            depth = depth[:, :, SLAB_Y0:SLAB_Y0 + SLAB_H].contiguous()
    return _rig(base["cams"], depth, geom, full_hw if whole else (SLAB_H, w), A_SRC, 0 if whole else SLAB_Y0)


def partial_rig():
    """PROJ, four views (launched 2 + 2), the matrix rig's two cameras and two milder ones."""
    base = matrix_rig("proj", False)
    cams = torch.zeros(4, 2, 18)
    cams[:2] = base["cams"]
    for b in range(2):
        cams[2, b, :12] = torch.tensor([0.98, -0.02, 0.7, 0.03, 1.01, -0.2 + 0.3 * b, -0.002, 0.004, 1.0, -0.4, 0.3, 0.03])
        cams[3, b, :12] = torch.tensor([1.2, 0.0, -0.3 * b, 0.0, 1.15, 0.6, 0.006, 0.0, 1.0, 0.8, -0.5 + 0.2 * b, -0.04])
    return _rig(cams, base["depth"], "proj", A_REF, A_SRC)


def all_rigs():
    """(name, rig) of every rig the GPU tests launch: the CPU tests assert the fragile cap on each."""
    for geom in ("proj", "homog"):
        for pp in (False, True):
            yield f"A {geom}{' per-pixel' if pp else ''}", matrix_rig(geom, pp)
    for kernel in POLICY:
        for mode in B_MODES:
            yield f"B {kernel} {mode}", zoom_rig(kernel, mode)
    for D in C_SHAPES:
        yield f"C D={D}", range_rig(D)
    yield "D 16 views", many_views_rig()
    yield "D narrow source", narrow_source_rig()
    for which in ("smaller", "larger"):
        yield f"D {which} source", sized_source_rig(which)
    for geom in ("proj", "homog"):
        for pp in (False, True):
            yield f"D slab {geom}{' per-pixel' if pp else ''}", slab_rig(geom, pp)
    yield "D partial", partial_rig()
