"""GPU: view covisibility (pscv_view_covisibility, csrc/view_covis.hip) against the numpy rule of tests/_covisibility_ref.py.
For every ordered pair and both counters |gpu - reference| <= the pair's borderline count (samples a last-bit difference could
decide the other way; tests/test_covisibility_cpu.py caps their share at 1 % per scene), and the diagonal is exactly 0.  Also an
empty view, a camera turned away (q_z <= 0), more targets than one LDS chunk, determinism, a side stream and the argument errors."""
import functools

import numpy as np
import pytest
import torch

from tests import _covisibility_ref as VR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from wild_deep_mvs_amd import _lib as L, ops
    L.lib()
    return L, ops


@functools.lru_cache(maxsize=None)
def _case(name):
    """(scene, cams, stride, reference counts, borderline, valid samples): computed once, shared, never written to."""
    make, stride = VR.GPU_CASES[name]
    sc = make()
    cams = VR.cams_of(sc)
    counts, border, nvalid = VR.covisibility([d.numpy() for d in sc["depths"]], cams.numpy(), stride=stride, max_depth_error=VR.MAX_DEPTH_ERROR)
    for a in (counts, border, nvalid):
        a.setflags(write=False)
    return sc, cams, stride, counts, border, nvalid


def _gpu(ops, name):
    sc, cams, stride, *_ = _case(name)
    out = ops.view_covisibility([d.cuda() for d in sc["depths"]], cams.cuda(), stride=stride, max_depth_error=VR.MAX_DEPTH_ERROR)
    assert out.dtype == torch.int32 and out.is_cuda and tuple(out.shape) == (len(sc["depths"]),) * 2 + (2,)
    return out.cpu().numpy().astype(np.int64)


def _check(got, want, border):
    V = want.shape[0]
    assert not got[np.arange(V), np.arange(V)].any(), "the diagonal is 0"
    diff = np.abs(got - want)
    bad = np.argwhere(diff > border[:, :, None])
    assert len(bad) == 0, f"{len(bad)} counters off by more than their borderline count, first (v, u, k) = {bad[0].tolist()}: " \
                          f"gpu {got[tuple(bad[0])]} reference {want[tuple(bad[0])]} borderline {border[bad[0][0], bad[0][1]]}"
    return int(diff.sum())


@pytest.mark.parametrize("name", ["v5_s1", "v5_s3"])
def test_counts_match_the_rule_on_ragged_views(env, name):
    L, ops = env
    sc, _, stride, want, border, nvalid = _case(name)
    assert any(d.shape[0] % 3 or d.shape[1] % 3 for d in sc["depths"]) and len({tuple(d.shape) for d in sc["depths"]}) > 1
    got = _gpu(ops, name)
    off = _check(got, want, border)
    print(f"{name}: seen {want[..., 0].sum()} consistent {want[..., 1].sum()} borderline {border.sum()} |gpu - ref| total {off}")
    assert want[..., 1].sum() > 0.5 * want[..., 0].sum() > 0 and (got[..., 1] <= got[..., 0]).all()
    assert (got[..., 0].max(axis=1) <= nvalid).all()


def test_a_view_without_depth_is_seen_but_sees_and_confirms_nothing(env):
    L, ops = env
    _, _, _, want, border, nvalid = _case("v5_zero")
    got = _gpu(ops, "v5_zero")
    _check(got, want, border)
    z = 2
    assert nvalid[z] == 0 and not got[z].any()                                   # its row
    others = [v for v in range(5) if v != z]
    assert (got[others, z, 0] > 0).all() and not got[:, z, 1].any()             # its column: seen, never consistent


def test_a_camera_turned_away_shares_nothing(env):
    L, ops = env
    _, _, _, want, border, nvalid = _case("v5_turned")
    got = _gpu(ops, "v5_turned")
    _check(got, want, border)
    assert nvalid[1] > 0 and not got[1].any() and not got[:, 1].any()            # q_z <= 0 both ways
    assert got[0, 2, 0] > 0


def test_more_targets_than_one_chunk_and_the_lists(env):
    """V = 70: the 64 targets of one LDS chunk (VC_CHUNK) and a second chunk of 6, and more views than CHECK_NUM_IMAGES = 50."""
    from wild_deep_mvs_amd.utils.colmap_model import overlap_from_covisibility
    L, ops = env
    _, _, _, want, border, _ = _case("v70")
    V = want.shape[0]
    assert V > VR.CHUNK and V > 50
    got = _gpu(ops, "v70")
    _check(got, want, border)
    assert got[:, VR.CHUNK:, 1].any() and got[VR.CHUNK:, :, 1].any()             # the second chunk counted, as source and target
    lg, lr = overlap_from_covisibility(got, 50), overlap_from_covisibility(want, 50)
    assert max(len(l) for l in lr) == 50
    # A GPU count lies in [reference - borderline, reference + borderline] of its pair.  The view at position k of a list is fixed
    # when exactly k other counts lie wholly above its interval and all the rest wholly below: there the lists must agree.
    checked = 0
    for v in range(V):
        others = np.array([u for u in range(V) if u != v])
        lo, hi = want[v, others, 1] - border[v, others], want[v, others, 1] + border[v, others]
        where = {int(u): i for i, u in enumerate(others)}
        for k, u in enumerate(lr[v]):
            i = where[u]
            if (lo > hi[i]).sum() == k and (hi < lo[i]).sum() == len(others) - 1 - k:
                assert len(lg[v]) > k and lg[v][k] == u, (v, k)
                checked += 1
    print(f"v70: {checked} of {sum(len(l) for l in lr)} list positions are fixed by the reference and were compared")
    assert checked > 300


def test_two_calls_give_identical_counts(env):
    L, ops = env
    a, b = _gpu(ops, "v70"), _gpu(ops, "v70")
    assert np.array_equal(a, b)
    assert np.array_equal(_gpu(ops, "v5_s1"), _gpu(ops, "v5_s1"))


def test_side_stream_beside_a_busy_default_stream(env):
    L, ops = env
    sc, cams, stride, *_ = _case("v70")
    depths, cams = [d.cuda() for d in sc["depths"]], cams.cuda()
    solo = ops.view_covisibility(depths, cams, stride=stride, max_depth_error=VR.MAX_DEPTH_ERROR)
    a = torch.randn(2048, 2048, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    for _ in range(20):
        a = (a @ a).clamp_(-1.0, 1.0)                                            # the default stream stays busy
    with torch.cuda.stream(side):
        beside = ops.view_covisibility(depths, cams, stride=stride, max_depth_error=VR.MAX_DEPTH_ERROR)
    side.synchronize()
    got = beside.cpu()
    torch.cuda.synchronize()
    assert torch.equal(got, solo.cpu())


def test_argument_errors(env):
    L, ops = env
    sc, cams, *_ = _case("v5_s1")
    depths, cams_d = [d.cuda() for d in sc["depths"]], cams.cuda()
    with pytest.raises(L.PscvError, match="n_views=1 < 2"):
        ops.view_covisibility(depths[:1], cams_d[:1], max_depth_error=0.01)
    with pytest.raises(L.PscvError, match="stride=0 < 1"):
        ops.view_covisibility(depths, cams_d, stride=0, max_depth_error=0.01)
    with pytest.raises(L.PscvError, match="max_depth_error"):
        ops.view_covisibility(depths, cams_d, max_depth_error=1.5)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        ops.view_covisibility(sc["depths"], cams_d, max_depth_error=0.01)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        ops.view_covisibility(depths, cams, max_depth_error=0.01)
    with pytest.raises(ValueError):
        ops.view_covisibility(depths, cams_d[:4], max_depth_error=0.01)          # one camera block per view
    # the C entry point checks its pointers and the workspace itself
    lib = L.lib()
    assert lib.pscv_view_covisibility_workspace(1) == -1 and lib.pscv_view_covisibility_workspace(70) >= 70 * 16
    assert lib.pscv_view_covisibility(None, None, 2, None, 1, 0.01, None, None, 0, None) == -1
    assert b"null pointer" in lib.pscv_last_error()
    torch.cuda.synchronize()
