"""What tests/test_gpu_geo_filter_ref.py and tests/test_gpu_filter.py share: the kernel's per-pair decisions (one launch per source)
and their comparison with the float64 reference of tests/_geo_filter_ref.py."""
import torch

import _geo_filter_ref as GR


def pair_counts(ops, sc, p):
    """[N,3,h,w] int64: the kernel's (depth, disp, geo) decisions of every pair, one launch per source"""
    depth = sc["depth"].cuda()
    out = []
    for i, s in enumerate(sc["src_depth"]):
        sel = [0, i + 1]
        cams = ops.geo_filter_cams(sc["K"][sel], sc["R"][sel], sc["t"][sel]).cuda()
        *_, c = ops.geo_filter(depth, [s.cuda()], cams, max_reproj_error=p[0], depth_threshold=p[1], min_tri_angle=p[2],
                               num_consistent=2, want_counts=True)
        out.append(c.cpu().long())
    return torch.stack(out).numpy()


def check_pairs(tag, got, r):
    """got [N,3,h,w] against the reference dict ``r``; prints the [parity] line"""
    assert got.min() >= 0 and got.max() <= 1, f"{tag}: a single-source count outside {{0, 1}}"
    worst = {}
    for j, k in enumerate(("depth", "disp", "geo")):
        bad = (got[:, j].astype(bool) != r[k]) & r[k + "_decided"]
        worst[k] = int(bad.sum())
    share, geo_share = GR.undecided_share(r)
    und = sum(int((~r[k + "_decided"]).sum()) for k in ("depth", "disp", "geo"))
    und_diff = sum(int(((got[:, j].astype(bool) != r[k]) & ~r[k + "_decided"]).sum()) for j, k in enumerate(("depth", "disp", "geo")))
    print(f"[parity] geo filter {tag}: {r['disp'].size} pairs, undecided {share:.3e} of the triples (geo {geo_share:.3e}); decided pairs that "
          f"differ {worst}; undecided decisions on the other side of the reference's nominal value {und_diff} of {und}", flush=True)
    assert share <= GR.UNDECIDED_CAP
    assert not any(worst.values()), f"{tag}: the kernel differs from the float64 reference on decided pairs: {worst}"
