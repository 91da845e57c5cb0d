"""numpy restatement of the view covisibility ("Overlap without a sparse model"), the yardstick of
csrc/view_covis.hip, and the scenes its tests share.

Geometry is float64 from the float32 inputs in the kernel's operation order (``unproject`` / ``project`` / ``round_away`` /
``depth_ok`` of tests/_colmap_fusion_ref.py: the rule is phase A's), vectorised per ordered pair of views.  Next to the counts the
reference reports, per pair, how many samples are BORDERLINE, i.e. could be decided the other way by a last-bit difference:
  * a projected coordinate within ``TOL_PX`` of a rounding boundary (a half-integer) or of an image edge (-0.5, size - 0.5),
    for projections in front of the camera that land in or at the rim of the target;
  * |q_z| < ``TOL_Z``;
  * a depth ratio |q_z - d_u| / d_u within ``TOL_RATIO`` of the threshold.
A GPU count may differ from the reference's by at most that number; tests/test_covisibility_cpu.py caps its share at 1 %."""
from __future__ import annotations

import numpy as np
import torch

from tests import _colmap_fusion_ref as CR

TOL_PX, TOL_Z, TOL_RATIO = 1e-3, 1e-6, 1e-5


def view_samples(depth, cam, stride):
    """World points (X, Y, Z) of the samples of one view: rows and columns that are multiples of ``stride``, valid depth."""
    depth = np.asarray(depth, dtype=np.float32)
    h, w = depth.shape
    rows, cols = np.meshgrid(np.arange(0, h, stride), np.arange(0, w, stride), indexing="ij")
    d = depth[::stride, ::stride]
    ok = CR.depth_ok(d)
    return CR.unproject(cam, cols[ok].astype(np.float64), rows[ok].astype(np.float64), d[ok].astype(np.float64))


def pair_counts(X, Y, Z, cam_u, depth_u, e):
    """(seen, consistent, borderline) of the samples (X, Y, Z) in target view u."""
    h, w = depth_u.shape
    with np.errstate(all="ignore"):
        x, y, z = CR.project(cam_u, X, Y, Z)
        pu, pv = x / z, y / z
        front = (z > 0.0) & (np.abs(pu) < CR.PIX_LIMIT) & (np.abs(pv) < CR.PIX_LIMIT)
        col, row = CR.round_away(np.where(front, pu, -1.0)), CR.round_away(np.where(front, pv, -1.0))
    inside = front & (col >= 0) & (col < w) & (row >= 0) & (row < h)
    du = np.zeros(len(X), dtype=np.float32)
    du[inside] = depth_u[row[inside].astype(np.int64), col[inside].astype(np.int64)]
    okd = inside & CR.depth_ok(du)
    dd = np.where(okd, du.astype(np.float64), 1.0)
    with np.errstate(all="ignore"):
        ratio = np.abs((z - dd) / dd)
    cons = okd & (ratio <= e)
    tiny = ~(np.abs(z) >= TOL_Z)                                   # (NaN counts as borderline too)
    near_half = lambda p: np.abs(np.abs(p - np.floor(p)) - 0.5) < TOL_PX      # image edges are half-integers as well
    rim = (pu > -0.5 - TOL_PX) & (pu < w - 0.5 + TOL_PX) & (pv > -0.5 - TOL_PX) & (pv < h - 0.5 + TOL_PX)
    with np.errstate(all="ignore"):
        b_round = front & rim & (near_half(pu) | near_half(pv))
    b_depth = okd & (np.abs(ratio - e) < TOL_RATIO)
    return int(inside.sum()), int(cons.sum()), int((tiny | b_round | b_depth).sum())


def covisibility(depths, cams, *, stride=4, max_depth_error):
    """depths V x [h_v, w_v] float32 (arrays or CPU tensors), cams [V,30] -> (counts int64 [V,V,2], borderline int64 [V,V],
    valid samples int64 [V])."""
    depths = [np.asarray(d, dtype=np.float32) for d in depths]
    cams = np.asarray(cams, dtype=np.float64)
    V = len(depths)
    e = float(np.float32(max_depth_error))
    counts, border, nvalid = np.zeros((V, V, 2), np.int64), np.zeros((V, V), np.int64), np.zeros(V, np.int64)
    for v in range(V):
        X, Y, Z = view_samples(depths[v], cams[v], stride)
        nvalid[v] = len(X)
        if len(X) == 0:
            continue
        for u in range(V):
            if u != v:
                counts[v, u, 0], counts[v, u, 1], border[v, u] = pair_counts(X, Y, Z, cams[u], depths[u], e)
    return counts, border, nvalid


def covisibility_like_op(depths, cams, *, stride=4, max_depth_error):
    """The reference behind the signature of ``ops.view_covisibility`` (tensors in, an int32 tensor out): what the CPU tests
    monkey-patch the op with."""
    counts, _, _ = covisibility([d.cpu().numpy() for d in depths], cams.cpu().numpy(), stride=stride, max_depth_error=max_depth_error)
    return torch.from_numpy(counts.astype(np.int32))


# ---- the scenes of tests/test_gpu_covisibility*.py (tests/test_covisibility_cpu.py checks the borderline cap on each) -----------
MAX_DEPTH_ERROR = 0.01
CHUNK = 64                      # VC_CHUNK of csrc/view_covis.hip: V = 70 spans two chunks


def cams_of(sc):
    from wild_deep_mvs_amd import ops
    return ops.geo_filter_cams(sc["K"], sc["R"], sc["t"])


def _base(V=5, H=24, W=32, **kw):
    from wild_deep_mvs_amd import synthetic
    return synthetic.make_permuted_yfcc_fusion_scene(V, H, W, seed=3, perm_seed=1, **kw)


def scene_plain():
    return _base()


def scene_zero_view(view=2):
    sc = _base()
    sc["depths"][view] = torch.zeros_like(sc["depths"][view])
    return sc


def scene_turned_view(view=1):
    """One camera turned by 180 degrees about its own y axis (centre kept): R' = D R, t' = D t with D = diag(-1, 1, -1).  Its depth
    map stays, so its points lie behind every other camera, and every other view's points lie behind it."""
    sc = _base()
    D = torch.diag(torch.tensor([-1.0, 1.0, -1.0]))
    sc["R"][view] = D @ sc["R"][view]
    sc["t"][view] = D @ sc["t"][view]
    return sc


def scene_many():
    return _base(V=70, H=8, W=12)


def scene_fusion():
    """The rig of tests/test_gpu_covisibility_fusion.py: 64 shuffled views, spaced so wide that only nearby views share surface."""
    from wild_deep_mvs_amd import synthetic
    return synthetic.make_permuted_yfcc_fusion_scene(64, 24, 32, seed=5, perm_seed=2, spacing=FUSION_SPACING)


FUSION_SPACING = 1.5
FUSION_KW = dict(max_depth_error=MAX_DEPTH_ERROR, max_reproj_error=1.0, min_num_pixels=3)
FUSION_STRIDE = 4

# name: (scene builder, stride)
GPU_CASES = {"v5_s1": (scene_plain, 1), "v5_s3": (scene_plain, 3), "v5_zero": (scene_zero_view, 1), "v5_turned": (scene_turned_view, 1),
             "v70": (scene_many, 1), "fusion64": (scene_fusion, FUSION_STRIDE)}
