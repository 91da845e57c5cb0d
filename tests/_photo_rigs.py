"""Hand-written rigs of tests/test_gpu_photo_ref.py, apart from it so that tests/test_photo_ref_cpu.py can check every one WITHOUT a
GPU: each reaches the regime it is named for (``check``: asserted on the float64 reference of _photo_ref.py) and keeps its fragile
share under FRAGILE_CAP.  Matrices are literals: inv_ref [B,4,4] maps (x d, y d, d, 1) to a point, proj [B,S,4,4] maps the point to
(q_x, q_y, q_z); no builder of the package stands between these numbers and the kernel.  Images are uniform in [0,1], depth jitters."""
import torch

import _photo_ref as R

NAN, INF = float("nan"), float("inf")


def _m(rows):
    return torch.tensor(rows, dtype=torch.float32)


def _inv_ref(b):
    return _m([[1.0, 0.01 + 0.02 * b, 0.0, 0.02], [-0.02, 1.0 - 0.01 * b, 0.0, 0.01 * b], [0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 1.0]])


def _view(ax, ay, cx, cy, tx, ty, zx=0.0, zy=0.0, tz=0.0):
    """q = (ax X + cx Z + tx, ay Y + cy Z + ty, zx X + zy Y + Z + tz): zoom a, shift c, parallax t / depth, tilt z."""
    return _m([[ax, 0.02, cx, tx], [-0.015, ay, cy, ty], [zx, zy, 1.0, tz], [0.0, 0.0, 0.0, 1.0]])


def _rig(name, hw, views, C=3, seed=0, depth=None, inv_ref=None, amp=0.2):
    """views[b][s] = a 4x4; depth defaults to 2 (1 +- amp / 2) per pixel."""
    B, S = len(views), len(views[0])
    h, w = hw
    g = torch.Generator().manual_seed(1000 + seed)
    rig = {"name": name, "hw": hw,
           "proj": torch.stack([torch.stack(v) for v in views]).contiguous(),
           "inv_ref": torch.stack([_inv_ref(b) for b in range(B)]) if inv_ref is None else inv_ref,
           "depth": (2.0 + 0.3 * torch.arange(B).view(B, 1, 1)) * (1.0 + amp * (torch.rand(B, h, w, generator=g) - 0.5)) if depth is None else depth,
           "src": torch.rand(B, S, C, h, w, generator=g), "src_depth": 1.5 + torch.rand(B, S, h, w, generator=g),
           "grad": torch.randn(B, S, C, h, w, generator=g)}
    rig["depth"] = rig["depth"].float().contiguous()
    return rig


def _flows(rig):
    return R.flows(rig["depth"], rig["inv_ref"], rig["proj"])


def regimes(rig, fl=None):
    return (fl or _flows(rig))["regime"]


def taps_inside(rig, fl=None):
    """Number of the four taps inside the image, [B,S,h,w]."""
    fl = fl or _flows(rig)
    h, w = rig["hw"]
    ix, iy = R.index_of(fl["gx"], 0 * fl["gx"], w)[0], R.index_of(fl["gy"], 0 * fl["gy"], h)[0]
    x0, y0 = torch.floor(ix), torch.floor(iy)
    nx = ((x0 >= 0) & (x0 < w)).long() + ((x0 + 1 >= 0) & (x0 + 1 < w)).long()
    ny = ((y0 >= 0) & (y0 < h)).long() + ((y0 + 1 >= 0) & (y0 + 1 < h)).long()
    return nx * ny, ix, iy


def fragile_shares(rig):
    f = R.fragile(rig["depth"], rig["inv_ref"], rig["proj"])
    return {k: float(v.double().mean()) for k, v in f.items()}


# ---- free: sub-pixel shift and zoom ------------------------------------------------------------------------------------------------
def free(hw, S, C, B, seed=0):
    views = [[_view(1.03 - 0.02 * s + 0.01 * b, 0.98 + 0.015 * s, 0.37 + 0.2 * s - 0.1 * b, 0.61 - 0.15 * s, 0.8 - 0.5 * s + 0.3 * b,
                    -0.6 + 0.4 * s, zx=0.002 * s, zy=-0.003 * b, tz=0.05 * s) for s in range(S)] for b in range(B)]
    return _rig(f"free {hw[0]}x{hw[1]} S{S} C{C} B{B}", hw, views, C=C, seed=seed)


def check_free(rig):
    fl = _flows(rig)
    n, _, _ = taps_inside(rig, fl)
    assert float((regimes(rig, fl) == 0).double().mean()) == 1.0 and float((n == 4).double().mean()) > 0.3
    if rig["proj"].shape[0] > 1:
        assert not torch.equal(rig["proj"][0], rig["proj"][1]) and not torch.equal(rig["inv_ref"][0], rig["inv_ref"][1])


FREE_CASES = [((5, 7), 1, 1, 1), ((5, 7), 4, 3, 3), ((16, 24), 1, 4, 1), ((16, 24), 4, 3, 1), ((9, 33), 4, 1, 3), ((9, 33), 1, 3, 1),
              ((16, 24), 4, 4, 3)]


# ---- border and mask edge: a zoom about the centre pushes samples out on all four sides --------------------------------------------
def zoomed(name, zoom, hw=(9, 13), seed=1):
    h, w = hw
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    views = [[_view(zoom + 0.01 * s, zoom - 0.01 * s, cx * (1 - zoom) + 0.3 * s, cy * (1 - zoom) - 0.2 * s, 0.3, -0.2) for s in range(2)]]
    return _rig(name, hw, views, seed=seed)


def border():
    """Near-identity maps: under align_corners=False the (size-1)-normalised flows already put the outermost rows and columns half a
    texel outside (two taps out on every side, three at the corners); shifted views add bands with all four taps outside."""
    views = [[_view(1.0, 1.0, cx, cy, 0.1, -0.1) for cx, cy in ((0.0, 0.0), (-1.4, -1.3), (1.4, 1.3), (-0.6, 0.7))]]
    return _rig("border", (9, 13), views, seed=1)


def check_border(rig):
    """An axis-aligned image loses its taps by rows and columns: 2 (a side), 3 (a corner) or 4 taps can be outside, never exactly 1."""
    n, ix, iy = taps_inside(rig)
    h, w = rig["hw"]
    for side in (ix < 0, ix > w - 1, iy < 0, iy > h - 1):
        assert int(((n == 2) & side).sum()) >= 4 and int(((n == 0) & side).sum()) >= 4, rig["name"]
    assert int((n == 1).sum()) >= 4 and int((n == 4).sum()) >= 20


def mask_edge():
    return zoomed("mask edge", 1.12, hw=(16, 24), seed=2)


def check_mask_edge(rig):
    fl = _flows(rig)
    for g in (fl["gx"], fl["gy"]):
        assert int((g > 1).sum()) >= 8 and int((g < -1).sum()) >= 8 and int((g.abs() < 1).sum()) >= 100
    assert float((regimes(rig, fl) == 0).double().mean()) == 1.0


# ---- clamp: |g| > 10 in x only, in y only, in both ---------------------------------------------------------------------------------
def clamp():
    h, w = 12, 16
    views = [[_view(14.0, 1.0, -40.0, 0.3, 0.5, 0.4),          # x zoom about column ~3: clamped left and right, free in between
              _view(1.0, 15.0, 0.4, -70.0, -0.4, 0.6),         # y only
              _view(13.0, 14.0, -60.0, -50.0, 0.5, 0.5)]]      # both, x only, y only and neither in one view
    return _rig("clamp", (h, w), views, seed=3)


def check_clamp(rig):
    fl = _flows(rig)
    r = regimes(rig, fl)
    for s, want in ((0, (R.XCL,)), (1, (R.YCL,)), (2, (R.XCL, R.YCL, R.XCL | R.YCL))):
        for code in want:
            assert int((r[:, s] == code).sum()) >= 20, (rig["name"], s, code)
    assert int((r == 0).sum()) >= 20
    xo = r == R.XCL                                      # the gradient is zero in the clamped axis ONLY
    assert bool((fl["dgx"][xo] == 0).all()) and bool((fl["dgy"][xo] != 0).all())


# ---- behind for part of the image: the plane of depth is cut by the source camera's image plane -------------------------------------
def part_behind():
    views = [[_view(1.02, 0.99, 0.3, 0.2, 0.5, -0.4, zx=-0.23), _view(1.0, 1.01, -0.2, 0.4, 0.3, 0.3, zy=-0.31),
              _view(1.01, 1.0, 0.1, 0.1, 0.2, 0.2)]]
    return _rig("part behind", (10, 14), views, seed=4)


def check_part_behind(rig):
    fl = _flows(rig)
    r = regimes(rig, fl)
    for s in (0, 1):
        share = float(((r[:, s] & R.BEHIND) > 0).double().mean())
        assert 0.2 < share < 0.8, (s, share)
    assert int((r[:, 2] & R.BEHIND).sum()) == 0
    n, _, _ = taps_inside(rig, fl)
    assert int(((r[:, :2] == 0) & (n[:, :2] == 4)).sum()) >= 20


# ---- z clamp: a band with 0 < q_z <= 1e-6, its depth solved from the reference's own q_z(d) = alpha d + beta ------------------------
def z_clamp():
    h, w = 10, 24
    inv = _m([[1.0, 0.01, 0.0, 0.0], [-0.01, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 1.0]]).view(1, 4, 4)
    views = [[_m([[1.0, 0.0, 0.0, 3e-6], [0.0, 1.0, 0.0, 2e-6], [0.004, -0.003, 1.0, 0.0], [0.0, 0.0, 0.0, 1.0]]),
              _m([[0.9, 0.0, 0.2, 2e-6], [0.0, 1.1, -0.1, 1e-6], [-0.002, 0.005, 1.0, 0.0], [0.0, 0.0, 0.0, 1.0]])]]
    proj = torch.stack([torch.stack(v) for v in views])
    g = torch.Generator().manual_seed(77)
    depth = 2.0 * (1.0 + 0.2 * (torch.rand(1, h, w, generator=g) - 0.5))
    one, two = torch.ones(1, h, w), 2.0 * torch.ones(1, h, w)
    z1 = R.flows(one, inv, proj)["z"][:, 0]
    z2 = R.flows(two, inv, proj)["z"][:, 0]
    alpha, beta = z2 - z1, 2.0 * z1 - z2                                       # q_z of view 0 is affine in the depth
    target = (0.1 + 0.85 * torch.rand(1, h, w, generator=g).double()) * R.ZMIN   # inside (0, 1e-6], off both ends
    target[:, 5:7] *= 2.5                                                        # rows 5, 6: partly just ABOVE 1e-6 (free, steep)
    band = (target - beta) / alpha
    depth[:, 2:7] = band[:, 2:7].float()
    return _rig("z clamp", (h, w), views, seed=5, depth=depth, inv_ref=inv)


def check_z_clamp(rig):
    fl = _flows(rig)
    r = regimes(rig, fl)
    assert int(((r[:, 0] & R.ZCL) > 0).sum()) >= 20 and int(((r[:, 0] & (R.ZCL | R.XCL | R.YCL)) == R.ZCL).sum()) >= 20
    z = fl["z"][:, 0]
    assert int(((z > R.ZMIN) & (z < 3 * R.ZMIN)).sum()) >= 10
    zc = (r[:, 0] == R.ZCL)
    assert bool((fl["dgx"][:, 0][zc][1:].abs() > 1e3).all())                     # f = q / 1e-6: a live, steep gradient


PHOTO_RIGS = {"border": (border, check_border), "mask_edge": (mask_edge, check_mask_edge), "clamp": (clamp, check_clamp),
              "part_behind": (part_behind, check_part_behind), "z_clamp": (z_clamp, check_z_clamp)}
for _i, (_hw, _S, _C, _B) in enumerate(FREE_CASES):
    PHOTO_RIGS[f"free_{_hw[0]}x{_hw[1]}_S{_S}_C{_C}_B{_B}"] = ((lambda hw=_hw, S=_S, C=_C, B=_B, i=_i: free(hw, S, C, B, seed=10 + i)), check_free)


def photo_rig(name):
    make, check = PHOTO_RIGS[name]
    rig = make()
    check(rig)
    return rig


# ---- non-finite ---------------------------------------------------------------------------------------------------------------------
def non_finite_depth():
    rig = free((16, 24), 2, 3, 1, seed=30)
    d = rig["depth"]
    d[0, 3, 0], d[0, 8, 0], d[0, 12, 0] = NAN, INF, -INF             # column 0: x inf = NaN
    d[0, 5, 7], d[0, 9, 11], d[0, 13, 20], d[0, 15, 23] = NAN, INF, -INF, NAN
    rig["name"] = "non-finite depth"
    return rig


def non_finite_image():
    """A NaN texel and an inf texel under a fractional shift: no sample is near an integer position (asserted), so the set of
    samples that touch either texel is the same in fp32."""
    rig = free((16, 24), 2, 3, 1, seed=32)
    rig["src"][0, 0, 1, 6, 9], rig["src"][0, 1, 2, 10, 14] = NAN, INF
    rig["src_depth"][0, 0, 4, 4], rig["src_depth"][0, 1, 12, 20] = INF, NAN
    rig["name"] = "non-finite image"
    return rig


# ---- SSIM ---------------------------------------------------------------------------------------------------------------------------
SSIM_H, SSIM_W = (1, 3, 7, 8, 9, 17), (1, 5, 31, 32, 33, 65)
SSIM_NCR = ((1, 1, 1), (2, 3, 3), (3, 1, 4), (2, 3, 1), (1, 1, 3), (3, 1, 1), (2, 3, 4), (1, 1, 4), (3, 1, 3))   # (n1, rep, C)
SSIM_KINDS = ("random", "equal", "constant", "zeros", "scale255", "nan")


def ssim_cases(kind):
    """random: every size, (n1, rep, C) cycling so that each triple meets both tile edges; the other kinds at three sizes."""
    if kind == "random":
        return [(h, w) + SSIM_NCR[(i * len(SSIM_W) + j) % len(SSIM_NCR)] for i, h in enumerate(SSIM_H) for j, w in enumerate(SSIM_W)]
    return [(3, 5, 1, 1, 1), (9, 33, 2, 3, 3), (17, 65, 3, 1, 4)]


def ssim_inputs(kind, h, w, n1, rep, C, seed=0):
    g = torch.Generator().manual_seed(500 + seed + 7 * h + w)
    a, b = torch.rand(n1, C, h, w, generator=g), torch.rand(n1 * rep, C, h, w, generator=g)
    if kind == "equal":
        b = a.repeat_interleave(rep, dim=0).clone()
    elif kind == "constant":
        a, b = torch.full_like(a, 0.625), torch.full_like(b, 0.25)
    elif kind == "zeros":
        a, b = torch.zeros_like(a), torch.zeros_like(b)
    elif kind == "scale255":
        a, b = torch.floor(a * 256.0).clamp(max=255.0), torch.floor(b * 256.0).clamp(max=255.0)
    elif kind == "nan":
        b[-1, C - 1, h // 2, w // 2] = NAN
    go = torch.randn(n1 * rep, C, h, w, generator=g)
    return a.contiguous(), b.contiguous(), go.contiguous()


# ---- homography ---------------------------------------------------------------------------------------------------------------------
def _hrig(name, H, ref_hw, src_hw, c, seed):
    m = H.shape[0]
    g = torch.Generator().manual_seed(900 + seed)
    return {"name": name, "H": H.float().contiguous(), "ref_hw": ref_hw, "src_hw": src_hw,
            "img": torch.rand(m, src_hw[0], src_hw[1], c, generator=g), "grad": torch.randn(m, ref_hw[0], ref_hw[1], c, generator=g)}


def _base_H(ref_hw, src_hw, zoom=1.0, m=2):
    (h, w), (hs, ws) = ref_hw, src_hw
    return torch.stack([_m([[zoom * ws / w * (1.02 + 0.03 * b), 0.01, 0.3 - ws * (zoom - 1) / 2], [-0.01, zoom * hs / h * (0.98 - 0.02 * b), 0.4 * b - hs * (zoom - 1) / 2],
                            [1e-3, -1e-3 * (b + 1), 1.0]]) for b in range(m)])


def _per_pixel(H, ref_hw, seed, amp=0.02):
    g = torch.Generator().manual_seed(seed)
    m = H.shape[0]
    return (H.view(m, 1, 1, 3, 3) * (1.0 + amp * (torch.rand(m, *ref_hw, 3, 3, generator=g) - 0.5))).contiguous()


def homog(kind, per_pixel, c, ref_hw=(9, 13), src_hw=(7, 10), seed=0):
    """free / border (a zoom: samples leave on all four sides and cross the +-1.1 clamp) / behind (h_z changes sign across the
    image) / tiny_z (per-pixel only: a band with 0 < h_z <= 1e-9, numerators of the same scale so that the position stays inside)."""
    H = _base_H(ref_hw, src_hw, zoom={"free": 1.0, "border": 1.5}.get(kind, 1.0))
    if kind == "behind":
        H[:, 2] = _m([-0.23, 0.002, 1.0])
    if per_pixel:
        H = _per_pixel(H, ref_hw, 40 + seed)
        if kind == "tiny_z":
            H[:, 2:5] = 0.0
            H[:, 2:5, :, 0, 0], H[:, 2:5, :, 1, 1] = 0.4e-9 * src_hw[1] / ref_hw[1], 0.4e-9 * src_hw[0] / ref_hw[0]
            g = torch.Generator().manual_seed(41)
            H[:, 2:5, :, 2, 2] = (0.1 + 0.85 * torch.rand(H.shape[0], 3, ref_hw[1], generator=g)) * 1e-9
    rig = _hrig(f"homography {kind} pp{int(per_pixel)} c{c} {src_hw}->{ref_hw}", H, ref_hw, src_hw, c, seed)
    check_homog(rig, kind)
    return rig


def check_homog(rig, kind):
    ix, iy, _, _, hz, _ = R.homography_positions(rig["H"], rig["ref_hw"], rig["src_hw"])
    hs, ws = rig["src_hw"]
    inside = (ix > 0) & (ix < ws - 1) & (iy > 0) & (iy < hs - 1)
    if kind == "free" and ws > 3 and hs > 3:
        assert float(inside.double().mean()) > 0.6
    if kind == "border":
        for a, size in ((ix, ws), (iy, hs)):
            assert int((a == -0.05 * (size - 1)).sum()) >= 4 and int((a == 1.05 * (size - 1)).sum()) >= 4      # clamped at +-1.1
            assert int(((a < 0) & (a > -0.05 * (size - 1))).sum()) + int(((a > size - 1) & (a < 1.05 * (size - 1))).sum()) >= 2
        assert int(inside.sum()) >= 10
    if kind == "behind":
        share = float((hz <= 0).double().mean())
        assert 0.2 < share < 0.8 and int(inside.sum()) >= 10
    if kind == "tiny_z":
        tiny = (hz > 0) & (hz <= R.HZMIN)
        assert int(tiny.sum()) >= 20 and int((tiny & inside).sum()) >= 10


HOMOG_CASES = [("free", 0, 1), ("free", 1, 3), ("free", 0, 8), ("free", 1, 32), ("border", 0, 3), ("border", 1, 8), ("behind", 0, 32),
               ("behind", 1, 1), ("tiny_z", 1, 3)]
HOMOG_SMALL = [((5, 6), (1, 1)), ((5, 6), (2, 3)), ((4, 5), (1, 4)), ((4, 5), (3, 1))]


def collision(exact, c=3, ref_hw=(24, 40)):
    """Every reference pixel lands on the same four texels of a 2 x 2 source: a constant map H = [[0,0,u],[0,0,v],[0,0,1]].
    exact: u = v = 1 -> ix = iy = 0.5, weights 0.25, integer gradients: every partial sum is a multiple of 0.25 below 2^22, exact in
    fp32 in ANY order.  A per-pixel variant moves single pixels to u, v in {0, 1, 2} (weights 0, 0.5, 1)."""
    h, w = ref_hw
    u = 1.0 if exact else 0.83
    v = 1.0 if exact else 1.21
    H = _m([[0.0, 0.0, u], [0.0, 0.0, v], [0.0, 0.0, 1.0]]).view(1, 3, 3)
    if exact:
        H = H.view(1, 1, 1, 3, 3).repeat(1, h, w, 1, 1)
        g = torch.Generator().manual_seed(8)
        H[0, :, :, 0, 2] = torch.randint(0, 3, (h, w), generator=g).float()
        H[0, :, :, 1, 2] = torch.randint(0, 3, (h, w), generator=g).float()
    rig = _hrig(f"collision exact{int(exact)}", H, ref_hw, (2, 2), c, 60 + int(exact))
    if exact:
        g = torch.Generator().manual_seed(9)
        rig["grad"] = torch.randint(-8, 9, rig["grad"].shape, generator=g).float()
    ix, iy, _, _, _, _ = R.homography_positions(rig["H"], ref_hw, (2, 2))
    assert bool(((ix >= 0) & (ix <= 1) & (iy >= 0) & (iy <= 1)).all())
    if exact:
        assert bool(((ix * 2) == torch.round(ix * 2)).all()) and bool(((iy * 2) == torch.round(iy * 2)).all())
    return rig
