"""pscv_geo_filter (csrc/geo_filter.hip) held to the float64 reference of tests/_geo_filter_ref.py, decision by decision
(tests/test_geo_filter_ref_cpu.py checks the reference, its band and its cases without a GPU).

Per (source, pixel) pair: the kernel is launched once per source with n_src = 1, num_consistent = 2 and want_counts, so its three
counts ARE the pair's three decisions (depth, disp, geo).  They equal the reference on every decided pair; on an undecided pair they
are 0 or 1.  Nothing is exempt by the pixel.
The multi-source launch: its counts are the sums of the single-source launches exactly (the arithmetic per pair is the same), and its
masks are ``count >= num_consistent - 1`` exactly for num_consistent in {1, 2, 3, N + 1, N + 2}: the source loop, the camera table in
LDS, the per-source shapes and ``need``."""
import numpy as np
import pytest
import torch

import _geo_filter_ref as GR
from _geo_filter_cmp import check_pairs, pair_counts

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from wild_deep_mvs_amd import _lib as L, ops
    L.lib()
    return L, ops


@pytest.mark.parametrize("name", GR.GPU_CASES)
def test_geo_filter_pairs_and_multi_source_launch(env, name):
    L, ops = env
    sc = GR.make_case(name)
    N = len(sc["src_depth"])
    depth, src = sc["depth"].cuda(), [s.cuda() for s in sc["src_depth"]]
    cams = ops.geo_filter_cams(sc["K"], sc["R"], sc["t"]).cuda()
    assert np.array_equal(cams.cpu().double().numpy(), GR.cam_blocks(sc["K"], sc["R"], sc["t"]))       # the reference sees the kernel's inputs
    for _, p in GR.PARAMS:
        got = pair_counts(ops, sc, p)
        check_pairs(f"{name} {p}", got, GR.reference(sc, p))
        total = got.sum(0)
        for nc in sorted({1, 2, 3, N + 1, N + 2}):
            md, mp, mg, counts = ops.geo_filter(depth, src, cams, max_reproj_error=p[0], depth_threshold=p[1], min_tri_angle=p[2],
                                                num_consistent=nc, want_counts=True)
            c = counts.cpu().long().numpy()
            assert np.array_equal(c, total), f"{name} {p} nc={nc}: counts differ from the sum of the single-source launches at " \
                                             f"{int((c != total).sum())} entries"
            for j, m in enumerate((md, mp, mg)):
                assert np.array_equal(m.cpu().numpy(), total[j] >= nc - 1), f"{name} {p} nc={nc}: mask {j} is not count >= {nc - 1}"
        # masks without the counts buffer: the same bytes
        md2, mp2, mg2 = ops.geo_filter(depth, src, cams, max_reproj_error=p[0], depth_threshold=p[1], min_tri_angle=p[2], num_consistent=nc)
        assert torch.equal(md2, md) and torch.equal(mp2, mp) and torch.equal(mg2, mg)
