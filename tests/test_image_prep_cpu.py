"""CPU: the host side of the image preparation.  The numpy restatement tests/_lanczos_ref.py is the
yardstick of the GPU tests, so it is held here against the fixture tests/golden/views_tiny.npz (PIL's own output and the
reference's own dataset methods, tests/golden/gen_golden_views.py), against live PIL where PIL is installed, and against CPU
torch's nearest interpolation; ``ops.lanczos_tables``, the tables the kernels read, must be the restatement's."""
import functools
import os

import numpy as np
import pytest
import torch
from torch.nn import functional as F

from tests import _lanczos_ref as LR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RESIZE_CASES = ("down", "up", "h_only", "v_only", "taps", "grey", "one", "blocks")
# the GPU test's cases, (W, H, channels (0 = mode L), w, h)
LIVE_CASES = [(53, 37, 3, 32, 32), (47, 33, 3, 96, 64), (40, 40, 3, 17, 40), (40, 40, 3, 40, 17), (301, 200, 3, 5, 7),
              (64, 95, 0, 64, 64), (64, 95, 1, 64, 64), (29, 31, 3, 1, 1)]
TABLE_CASES = [(53, 32), (37, 32), (47, 96), (33, 64), (301, 5), (200, 7), (95, 64), (31, 1), (1600, 682), (1200, 512), (7, 7)]


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(os.path.join(GOLDEN, "views_tiny.npz")))


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name", RESIZE_CASES)
def test_restatement_equals_the_fixture(name):
    z = fixture()
    want = z[f"{name}_out"]
    got = LR.resize(z[f"{name}_in"], (want.shape[1], want.shape[0]))
    assert same_bits(got, want), f"{name}: {int((got != want).sum())} of {want.size} bytes differ"


def test_the_block_image_reaches_both_clamps():
    out = fixture()["blocks_out"]
    assert (out == 0).any() and (out == 255).any()


@pytest.mark.parametrize("W,H,c,w,h", LIVE_CASES)
def test_restatement_equals_live_pil(W, H, c, w, h):
    Image = pytest.importorskip("PIL.Image")
    img = LR.random_image(H, W, c, seed=W + h)
    pil = Image.fromarray(img[:, :, 0] if c == 1 else img)
    want = np.asarray(pil.resize((w, h), resample=Image.LANCZOS))
    got = LR.resize(img, (w, h))
    assert same_bits(got[:, :, 0] if c == 1 else got, want)


def test_restatement_equals_live_pil_on_step_edges():
    Image = pytest.importorskip("PIL.Image")
    img = LR.block_image(60, 70, 3, cell=4, seed=9)
    want = np.asarray(Image.fromarray(img).resize((43, 35), resample=Image.LANCZOS))
    assert (want == 0).any() and (want == 255).any()
    assert same_bits(LR.resize(img, (43, 35)), want)


@pytest.mark.parametrize("in_len,out_len", [(23, 17), (17, 40), (512, 512)])
def test_nearest_index_is_cpu_torchs(in_len, out_len):
    src = torch.arange(in_len, dtype=torch.float32).view(1, 1, 1, in_len)
    want = F.interpolate(src, size=(1, out_len), mode="nearest").view(-1).numpy().astype(np.int64)
    assert np.array_equal(LR.nearest_index(out_len, in_len), want)


def test_depth_mask_compares_in_fp32_like_torch():
    """The reference compares an fp32 tensor with float64 numbers from the ``.npz``: torch rounds the number to fp32 first."""
    lo, hi = np.float64(0.7), np.float64(1.3)                    # fp32(0.7) < 0.7 and fp32(1.3) > 1.3
    d = np.array([[np.float32(0.7), np.float32(1.3), 1.0, 0.5]], dtype=np.float32)
    t = torch.tensor(d)
    want = ((t >= lo) & (t < hi)).numpy()
    _, mask = LR.depth_nearest_crop(d, d.shape, (0, 0) + d.shape, lo, hi)
    assert np.array_equal(mask.astype(bool), want) and want.tolist() == [[True, False, True, False]]


@pytest.mark.parametrize("in_len,out_len", TABLE_CASES)
def test_tables_have_the_stated_ksize_and_sum_to_one(in_len, out_len):
    from wild_deep_mvs_amd import ops
    coeff, bounds, ksize = ops.lanczos_tables(in_len, out_len)
    fs = max(in_len / out_len, 1.0)
    assert ksize == 2 * int(np.ceil(3.0 * fs)) + 1
    assert coeff.dtype == np.int32 and coeff.shape == (out_len, ksize) and bounds.dtype == np.int32 and bounds.shape == (out_len, 2)
    first, n = bounds[:, 0].astype(np.int64), bounds[:, 1].astype(np.int64)
    assert (first >= 0).all() and (n >= 1).all() and (n <= ksize).all() and (first + n <= in_len).all()
    for o in range(out_len):
        assert not coeff[o, n[o]:].any()
        # every weight is rounded to the nearest integer: n errors of at most 1/2, plus the float64 rounding of the normalised sum
        assert abs(int(coeff[o].astype(np.int64).sum()) - (1 << 22)) <= n[o] / 2 + 1, (o, coeff[o])
    # an int32 accumulator holds 2^21 + 255 * the positive (or the negative) weights of any row
    wide = coeff.astype(np.int64)
    assert 255 * np.where(wide > 0, wide, 0).sum(1).max() + (1 << 21) < 2 ** 31 and 255 * np.where(wide < 0, -wide, 0).sum(1).max() < 2 ** 31
    want_c, want_b, want_k = LR.tables(in_len, out_len)
    assert want_k == ksize and np.array_equal(coeff, want_c) and np.array_equal(bounds, want_b)


def test_tables_are_cached_and_read_only():
    from wild_deep_mvs_amd import ops
    a, b = ops.lanczos_tables(53, 32), ops.lanczos_tables(53, 32)
    assert a[0] is b[0] and not a[0].flags.writeable and not a[1].flags.writeable
    with pytest.raises(ValueError):
        ops.lanczos_tables(5, 0)


@pytest.mark.parametrize("mode", ["train", "test"])
def test_prepare_view_restatement_equals_the_fixture(mode):
    z = fixture()
    height, width, multi = (int(v) for v in z["pv_params"])
    depth = z["pv_depth"] if mode == "train" else None
    im, K, r, d, m = LR.prepare_view(z["pv_img"], z["pv_K"], mode, height, width, multi, True, depth, tuple(z["pv_range"]))
    assert same_bits(im, z[f"pv_{mode}_im"]) and same_bits(K, z[f"pv_{mode}_K"]) and float(r) == float(z[f"pv_{mode}_r"])
    if mode == "train":
        assert same_bits(d, z["pv_train_depth"]) and same_bits(m, z["pv_train_mask"])
        lo, hi = (np.float32(v) for v in z["pv_range"])
        assert m[d == lo].all() and not m[d == hi].any() and (d == lo).any() and (d == hi).any()


@pytest.mark.parametrize("mode", ["train", "test"])
def test_prepare_view_k_equals_the_fixtures_bits(mode):
    """The package's own K (wild_deep_mvs_amd/data/views.py; host code, no device needed)."""
    from wild_deep_mvs_amd.data import views
    z = fixture()
    height, width, multi = (int(v) for v in z["pv_params"])
    H, W = z["pv_img"].shape[:2]
    r, size, (x0, y0, cw, ch) = views.view_geometry(W, H, mode, height, width, multi)
    K = views.crop_calib(x0, y0, views.rescale_calib(r, z["pv_K"]))
    assert same_bits(K, z[f"pv_{mode}_K"]) and float(r) == float(z[f"pv_{mode}_r"])
    assert (ch, cw) == z[f"pv_{mode}_im"].shape[1:]
    assert (r, size, (x0, y0, cw, ch)) == LR.view_geometry(W, H, mode, height, width, multi)


def test_view_geometry_rejects_what_the_reference_cannot_crop():
    from wild_deep_mvs_amd.data import views
    with pytest.raises(ValueError):
        views.view_geometry(100, 80, "val")
    with pytest.raises(ValueError):
        views.view_geometry(20, 80, "test")                      # no multiple of 32 in 20 columns
    with pytest.raises(ValueError):
        views.view_geometry(100, 80, "train", resize=False)      # smaller than the 512 x 512 window


def test_resized_size_is_the_packages():
    from wild_deep_mvs_amd import preprocess
    for size in [(640, 480), (1600, 1067), (1067, 1600), (513, 700), (512, 512), (3000, 2000)]:
        assert LR.resized_size(size, 512) == preprocess.getResizedSize(size, 512)


def test_ops_raise_without_a_device():
    from wild_deep_mvs_amd import ops
    with pytest.raises(RuntimeError):
        ops.resize_lanczos_u8(torch.zeros((4, 4, 3), dtype=torch.uint8), (2, 2))
    with pytest.raises(RuntimeError):
        ops.depth_nearest_crop(torch.zeros((4, 4)), (2, 2))
