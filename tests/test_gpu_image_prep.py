"""GPU: the image preparation (csrc/image_resample.hip behind ops.resize_lanczos_u8 and ops.depth_nearest_crop,
wild_deep_mvs_amd/data/views.py:prepare_view, preprocess.py:resize_tuple_images).

PIL's resampling is integer arithmetic and the nearest resize is an index rule, so the bar is EQUALITY: ``torch.equal`` on the
uint8 images and on the bits of the fp32 ones, against the fixture tests/golden/views_tiny.npz (PIL's own output, the reference's
own dataset methods) and the numpy restatement tests/_lanczos_ref.py, which tests/test_image_prep_cpu.py holds against PIL.  The
GPU box needs no PIL.  Shapes are the smallest at which each path is taken: both passes, either pass alone, neither, windows on
and off the borders, one and three channels, more than one workgroup per axis, and one real size."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import _lanczos_ref as LR

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RESIZE_CASES = ("down", "up", "h_only", "v_only", "taps", "grey", "one", "blocks")


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from wild_deep_mvs_amd import _lib as L, ops
    L.lib()
    return L, ops


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(os.path.join(GOLDEN, "views_tiny.npz")))


@functools.lru_cache(maxsize=None)
def real_size():
    """(image 1200 x 1600 x 3, the restatement's 512 x 682 resize): computed once, never written to."""
    img = LR.random_image(1200, 1600, 3, seed=2)
    img[:, :, 1] = (np.add.outer(np.arange(1200), np.arange(1600)) // 7 % 256).astype(np.uint8)       # a smooth channel too
    want = LR.resize(img, (682, 512))
    img.setflags(write=False)
    want.setflags(write=False)
    return img, want


def _d(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()           # (a copy: the shared inputs are read-only)


def _equal(got, want):
    """Same shape, dtype and bits (fp32 compared as its 32-bit words)."""
    want = torch.from_numpy(np.array(want, order="C"))
    got = got.cpu()
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    return torch.equal(got.view(torch.int32), want.view(torch.int32)) if got.dtype == torch.float32 else torch.equal(got, want)


@pytest.mark.parametrize("name", RESIZE_CASES)
def test_resize_equals_pil(env, name):
    """down: non-integer down-scale on both axes; up: ksize 7, bounds clipped at both edges; h_only / v_only: one pass skipped;
    taps: about 260 taps per output; grey: mode L as [H,W]; one: 1 x 1; blocks: both clamps."""
    _, ops = env
    z = fixture()
    want = z[f"{name}_out"]
    if name == "blocks":
        assert (want == 0).any() and (want == 255).any()
    if name == "up":
        assert ops.lanczos_tables(47, 96)[2] == 7
    got = ops.resize_lanczos_u8(_d(z[f"{name}_in"]), (want.shape[1], want.shape[0]))
    assert got.is_cuda and got.is_contiguous()
    assert _equal(got, want), f"{name}: {int((got.cpu().numpy() != want).sum())} of {want.size} bytes differ from PIL"


def test_grey_with_a_channel_axis(env):
    _, ops = env
    z = fixture()
    got = ops.resize_lanczos_u8(_d(z["grey_in"][:, :, None]), (64, 64))
    assert tuple(got.shape) == (64, 64, 1) and _equal(got[:, :, 0], z["grey_out"])


@pytest.mark.parametrize("name,crop", [("down", (5, 7, 20, 11)), ("down", (0, 0, 9, 32)), ("up", (37, 51, 59, 13)),
                                       ("h_only", (3, 5, 11, 30)), ("v_only", (29, 0, 11, 17)), ("grey", (1, 2, 62, 61))])
def test_a_crop_is_the_slice_of_the_whole(env, name, crop):
    """Windows that touch no border, and windows that touch two (the top-left corner; the bottom-right corner)."""
    _, ops = env
    z = fixture()
    want = z[f"{name}_out"]
    x0, y0, w, h = crop
    got, f32 = ops.resize_lanczos_u8(_d(z[f"{name}_in"]), (want.shape[1], want.shape[0]), crop=crop, want_f32=True)
    assert _equal(got, want[y0:y0 + h, x0:x0 + w])
    assert _equal(f32, LR.to_f32_chw(want[y0:y0 + h, x0:x0 + w]))


@pytest.mark.parametrize("name", ["down", "h_only", "v_only", "grey"])
def test_f32_chw_is_numpys_division(env, name):
    _, ops = env
    z = fixture()
    want = z[f"{name}_out"]
    u8, f32 = ops.resize_lanczos_u8(_d(z[f"{name}_in"]), (want.shape[1], want.shape[0]), want_f32=True)
    chw = want[:, :, None] if want.ndim == 2 else want
    assert _equal(u8, want) and _equal(f32, np.ascontiguousarray((np.float32(chw) / np.float32(255)).transpose(2, 0, 1)))


def test_same_size_is_a_copy_a_crop_and_a_conversion(env):
    """Neither pass runs, as in PIL; every byte value goes through the fp32 table."""
    _, ops = env
    img = np.arange(7 * 300 * 3, dtype=np.int64).reshape(7, 300, 3).astype(np.uint8)
    assert len(np.unique(img)) == 256
    assert _equal(ops.resize_lanczos_u8(_d(img), (300, 7)), img)
    u8, f32 = ops.resize_lanczos_u8(_d(img), (300, 7), crop=(3, 2, 290, 4), want_f32=True)
    assert _equal(u8, img[2:6, 3:293]) and _equal(f32, LR.to_f32_chw(img[2:6, 3:293]))


def test_real_size_with_the_centre_crop(env):
    """1600 x 1200 -> 682 x 512 and its 512 x 512 centre window: several workgroups on both axes of both passes."""
    _, ops = env
    img, want = real_size()
    x0 = (682 - 512) // 2
    dev = _d(img)
    got, f32 = ops.resize_lanczos_u8(dev, (682, 512), crop=(x0, 0, 512, 512), want_f32=True)
    assert _equal(got, want[:, x0:x0 + 512]) and _equal(f32, LR.to_f32_chw(want[:, x0:x0 + 512]))
    assert _equal(ops.resize_lanczos_u8(dev, (682, 512)), want)


def test_depth_nearest_crop(env):
    """23 x 31 -> 37 x 50 with a window; depths exactly on min_d (inside) and on max_d (outside)."""
    _, ops = env
    rng = np.random.default_rng(4)
    lo, hi = 1.5, 6.25
    depth = rng.uniform(1.0, 7.0, (23, 31)).astype(np.float32)
    depth[::2, ::3] = lo
    depth[1::2, 1::3] = hi
    depth[3, 4] = np.nan
    crop = (2, 3, 33, 44)
    want_d, want_m = LR.depth_nearest_crop(depth, (37, 50), crop, lo, hi)
    assert (want_d == np.float32(lo)).any() and (want_d == np.float32(hi)).any() and np.isnan(want_d).any()
    assert want_m[want_d == np.float32(lo)].all() and not want_m[want_d == np.float32(hi)].any()
    got_d, got_m = ops.depth_nearest_crop(_d(depth), (37, 50), crop=crop, min_d=lo, max_d=hi)
    assert _equal(got_d, want_d) and _equal(got_m, want_m)
    whole_d, whole_m = ops.depth_nearest_crop(_d(depth), (37, 50), min_d=lo, max_d=hi)
    assert _equal(whole_d[2:35, 3:47].contiguous(), want_d) and _equal(whole_m[2:35, 3:47].contiguous(), want_m)
    # bounds that are not fp32 numbers are rounded to fp32, as torch does (tests/test_image_prep_cpu.py)
    d2 = np.array([[np.float32(0.7), np.float32(1.3), 1.0, 0.5]], dtype=np.float32)
    _, m2 = ops.depth_nearest_crop(_d(d2), (1, 4), min_d=np.float64(0.7), max_d=np.float64(1.3))
    assert m2.cpu().numpy().tolist() == [[1, 0, 1, 0]]


@pytest.mark.parametrize("mode", ["train", "test"])
def test_prepare_view_equals_the_reference(env, mode):
    from wild_deep_mvs_amd.data import views
    z = fixture()
    height, width, multi = (int(v) for v in z["pv_params"])
    kw = dict(depth=_d(z["pv_depth"]), depth_range=tuple(z["pv_range"])) if mode == "train" else {}
    im, K, r, d, m = views.prepare_view(_d(z["pv_img"]), z["pv_K"], mode, height, width, multi, **kw)
    assert im.is_cuda and _equal(im, z[f"pv_{mode}_im"])
    assert K.dtype == np.float32 and K.tobytes() == z[f"pv_{mode}_K"].tobytes() and float(r) == float(z[f"pv_{mode}_r"])
    if mode == "train":
        assert m.dtype == torch.bool and _equal(d, z["pv_train_depth"]) and _equal(m.to(torch.uint8), z["pv_train_mask"])
    else:
        assert d is None and m is None
        with pytest.raises(ValueError):
            views.prepare_view(_d(z["pv_img"]), z["pv_K"], "test", depth=_d(z["pv_depth"]), depth_range=(1.0, 2.0))


def test_prepare_view_without_resize_only_crops(env):
    from wild_deep_mvs_amd.data import views
    z = fixture()
    img = z["pv_img"]
    im, K, r, _, _ = views.prepare_view(_d(img), torch.from_numpy(z["pv_K"]), "train", 32, 40, resize=False)
    want_im, want_K, want_r, _, _ = LR.prepare_view(img, z["pv_K"], "train", 32, 40, do_resize=False)
    assert r == 1 == want_r and _equal(im, want_im) and K.tobytes() == want_K.tobytes()
    assert _equal(im, LR.to_f32_chw(img[14:46, 21:61]))


def test_resize_tuple_images(env):
    """Three images of different sizes and aspect ratios; minSize 64 keeps them small (landscape, portrait, nearly square)."""
    from wild_deep_mvs_amd import preprocess
    imgs = [LR.random_image(h, w, 3, seed=h) for w, h in [(150, 100), (90, 161), (131, 129)]]
    out, sizes = preprocess.resize_tuple_images([_d(a) for a in imgs], minSize=64)
    assert sizes.dtype == np.int64 and sizes.tolist() == [[96, 64], [64, 96], [64, 64]]
    assert sizes.tolist() == [list(LR.resized_size((a.shape[1], a.shape[0]), 64)) for a in imgs]
    for a, o, (w, h) in zip(imgs, out, sizes.tolist()):
        assert o.is_cuda and _equal(o, LR.resize(a, (w, h)))


def test_argument_errors(env):
    L, ops = env
    img = _d(fixture()["down_in"])
    with pytest.raises(ValueError):
        ops.resize_lanczos_u8(img[:, ::2], (8, 8))                               # not contiguous
    with pytest.raises(ValueError):
        ops.resize_lanczos_u8(img.to(torch.float32), (8, 8))                     # not uint8
    with pytest.raises(ValueError):
        ops.resize_lanczos_u8(_d(np.zeros((5, 5, 4), dtype=np.uint8)), (8, 8))   # RGBA
    with pytest.raises(ValueError):
        ops.resize_lanczos_u8(_d(np.zeros((5, 5, 2), dtype=np.uint8)), (8, 8))
    for size in [(0, 8), (8, 0), (-3, 8)]:
        with pytest.raises(ValueError):
            ops.resize_lanczos_u8(img, size)
    for crop in [(-1, 0, 4, 4), (0, -1, 4, 4), (5, 0, 4, 4), (0, 5, 4, 4), (0, 0, 0, 4), (0, 0, 4, 0), (0, 0, 9, 4)]:
        with pytest.raises(ValueError):
            ops.resize_lanczos_u8(img, (8, 8), crop=crop)
    with pytest.raises(RuntimeError):
        ops.resize_lanczos_u8(img.cpu(), (8, 8))
    depth = torch.ones((6, 7), device="cuda")
    with pytest.raises(ValueError):
        ops.depth_nearest_crop(depth.double(), (4, 4))
    with pytest.raises(ValueError):
        ops.depth_nearest_crop(depth, (0, 4))
    with pytest.raises(ValueError):
        ops.depth_nearest_crop(depth, (4, 4), crop=(1, 1, 4, 3))
    with pytest.raises(ValueError):
        ops.depth_nearest_crop(depth.t(), (4, 4))
    # the C ABI checks for itself
    out = torch.empty((4, 4, 3), dtype=torch.uint8, device="cuda")
    rc = L.lib().pscv_resample_u8_pass(img.data_ptr(), 53 * 3, 4, 53, 2, 1, None, None, 0, 53, 0, 4, out.data_ptr(), None, None, None)
    assert rc != 0 and "C=2" in L.lib().pscv_last_error().decode()
    rc = L.lib().pscv_resample_u8_pass(img.data_ptr(), 53 * 3, 4, 37, 3, 1, None, None, 0, 37, 35, 4, out.data_ptr(), None, None, None)
    assert rc != 0 and "outside" in L.lib().pscv_last_error().decode()


def test_two_runs_give_identical_bytes(env):
    _, ops = env
    z = fixture()
    dev = _d(z["taps_in"])
    a = ops.resize_lanczos_u8(dev, (97, 71), crop=(3, 2, 90, 60), want_f32=True)
    b = ops.resize_lanczos_u8(dev, (97, 71), crop=(3, 2, 90, 60), want_f32=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    assert _equal(a[0], LR.resize(z["taps_in"], (97, 71))[2:62, 3:93])
