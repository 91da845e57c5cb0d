"""What tests/test_gpu_photo_ref.py and the older GPU tests of the same kernels share: the per-kernel bounds (units of 2^-24 U, the
unit of tests/_photo_ref.py), the per-element comparison, and the checks of a function-level homography call."""
import torch

import _photo_ref as R

# (kernel, output): bound in units of 2^-24 U.            worst measured ratio (MI355X)        4 x worst
BOUND = {
    ("photo_warp", "z"): 8,                              # 1.81 (part behind)                      7.2
    ("photo_warp", "flows"): 7,                          # 1.56                                    6.3
    ("photo_warp", "warped"): 4,                         # 0.93                                    3.7
    ("photo_warp", "warped_depth"): 6,                   # 1.29                                    5.2
    ("photo_warp_bwd", "grad_depth"): 3,                 # 0.53                                    2.1
    ("ssim", "out"): 7,                                  # 1.56                                    6.2
    ("ssim_bwd", "grad"): 2,                             # 0.28                                    1.1
    ("homography_warp", "out"): 6,                       # 1.47 (3 x 1 source)                     5.9
    ("homography_warp_bwd", "grad"): 6,                  # 1.45 (behind, 32 channels)              5.8
}
CAP = {("photo_warp", "z"): 9, ("photo_warp", "flows"): 9, ("photo_warp", "warped"): 9, ("photo_warp", "warped_depth"): 9,
       ("ssim", "out"): 23, ("ssim_bwd", "grad"): 45, ("homography_warp", "out"): 7}      # the two backwards: per case (``cap=``)
assert all(BOUND[k] <= c for k, c in CAP.items())
BOUND[("photometricloss", "ssim")] = BOUND[("ssim", "out")]                    # the composition: the last kernel's bound, composed units
BOUND[("photometricloss", "grad_depth")] = BOUND[("photo_warp_bwd", "grad_depth")]
EPS = R.EPS


def compare(key, tag, got, ref, U, cap=None, exempt=None, coarse=None, table=None):
    """fp32 ``got`` against the float64 ``ref``: NaN and inf exactly where the reference has them; the rest within
    min(BOUND, cap) 2^-24 U (exactly equal where U is 0); ``exempt`` elements finite and within ``coarse``.
    ``table``: a dict that collects the worst ratio per key."""
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    nan, inf = torch.isnan(ref), torch.isinf(ref)
    assert torch.equal(torch.isnan(got), nan), f"{tag}: NaN at {int(torch.isnan(got).sum())} elements, reference at {int(nan.sum())}"
    assert torch.equal(got[inf], ref[inf]), f"{tag}: inf elements differ"
    fin = ~(nan | inf)
    strict = fin if exempt is None else fin & ~exempt
    err = (got - ref).abs()
    unit = EPS * U
    ratio = torch.where(unit > 0, err / unit, torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    worst = float(ratio[strict].max()) if bool(strict.any()) else 0.0
    if table is not None:
        table[key] = max(table.get(key, 0.0), worst)
    bound = BOUND[key] if cap is None else min(BOUND[key], cap)
    print(f"[parity] {tag}: worst ratio {worst:.3f} (bound {bound}), max abs err {float(err[strict].max()) if bool(strict.any()) else 0.0:.2e}"
          + (f", {int((exempt & fin).sum())} fragile" if exempt is not None else ""), flush=True)
    assert worst <= bound, f"{tag}: |got - ref| = {worst:.3f} x 2^-24 U at its worst element, bound {bound}"
    if exempt is not None and bool((exempt & fin).any()):
        e = exempt & fin
        assert bool(torch.isfinite(got[e]).all()) and bool((err[e] <= coarse[e]).all()), f"{tag}: a fragile element left its coarse bound"


def contributions(H, ref_hw, src_hw):
    """Largest number of reference pixels that add to one texel (taps outside the image are counted on a one-texel rim)."""
    ix, iy, _, _, _, _ = R.homography_positions(H, ref_hw, src_hw)
    hs, ws = src_hw
    m = ix.shape[0]
    cnt = torch.zeros(m, (hs + 2) * (ws + 2))
    x0, y0 = torch.floor(ix).long().clamp(-1, ws - 1) + 1, torch.floor(iy).long().clamp(-1, hs - 1) + 1
    for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
        cnt.scatter_add_(1, ((y0 + dy) * (ws + 2) + x0 + dx).view(m, -1), torch.ones(m, ix[0].numel()))
    return int(cnt.max())


def homography_call(tag, got, oracle, src, H, ref_hw, grad_out=None, got_grad=None):
    """One homography_warping call of the function-level API (NCHW tensors on the CPU; H [m,3,3] or [m,h,w,3,3]) against the float64
    reference per element, its input gradient too where given.  Returns the max_abs the fp32 ``oracle`` output can be held to for
    THESE inputs: the kernel's bound at its worst element plus the oracle's own distance from float64."""
    r = R.homography(src.detach().permute(0, 2, 3, 1), H, ref_hw)
    compare(("homography_warp", "out"), f"{tag} vs float64", got.detach().permute(0, 2, 3, 1), r["out"], r["U"])
    if got_grad is not None:
        gb = R.homography_bwd(grad_out.permute(0, 2, 3, 1), H, tuple(src.shape[2:]))
        compare(("homography_warp_bwd", "grad"), f"{tag} d input vs float64", got_grad.permute(0, 2, 3, 1), gb["grad"], gb["U"],
                cap=contributions(H, ref_hw, tuple(src.shape[2:])) + 4)
    own = float((oracle.detach().double().permute(0, 2, 3, 1) - r["out"]).abs().max())
    return BOUND[("homography_warp", "out")] * EPS * float(r["U"].max()) + own
