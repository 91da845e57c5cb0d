"""GPU: the training-view augmentation (csrc/image_augment.hip behind ops.augment_views, data/views.py:prepare_view(augment=...);
INTEGRATION.md section 2m).

The colour steps are PIL's byte arithmetic and the blur is a stated sequence of fp32 roundings, so the bar is EQUALITY of the fp32
bits: against the fixture tests/golden/augment_tiny.npz (PIL's own ImageEnhance outputs; the GPU box needs no PIL) and against the
numpy restatement tests/_augment_ref.py, which tests/test_augment_cpu.py holds against PIL.  Shapes are the smallest at which each
path is taken: axes of length 1 and 2 (where the reflection folds), more than one workgroup on both axes, windows on and off the
borders, several views in one call, and one image whose sum of L needs more than 32 bits."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import _augment_ref as AR
from tests import _lanczos_ref as LR

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ("bright", "bright_hi", "contrast", "clip", "bc", "cb", "half")
NAMES = {1: "brightness", 2: "contrast"}


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from wild_deep_mvs_amd import _lib as L, ops
    L.lib()
    return L, ops


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(os.path.join(GOLDEN, "augment_tiny.npz")))


@functools.lru_cache(maxsize=None)
def blocks_image():
    """70 x 131: two workgroups down, three across.  Read-only."""
    img = AR.random_image(70, 131, seed=8)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def blocks_blurred(mode):
    out = AR.blur32(AR.unit(blocks_image()), AR.motion_kernel(mode, 3))
    out.setflags(write=False)
    return out


def _d(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()           # (a copy: the shared inputs are read-only)


def _equal(got, want):
    """Same shape, dtype and bits (fp32 compared as its 32-bit words)."""
    want = torch.from_numpy(np.array(want, order="C"))
    got = got.cpu()
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    return torch.equal(got.view(torch.int32), want.view(torch.int32)) if got.dtype == torch.float32 else torch.equal(got, want)


def case_steps(z, name):
    return [(NAMES[int(o)], float(f)) for o, f in zip(z[f"{name}_ops"], z[f"{name}_factors"])]


@pytest.mark.parametrize("name", CASES)
def test_colour_steps_equal_pil(env, name):
    """Brightness alone (inside and above [0, 1]), contrast alone, the clip case, both orders, the mean of exactly x.5."""
    _, ops = env
    z = fixture()
    got = ops.augment_views(_d(z[f"{name}_in"][None]), [(case_steps(z, name), None)])
    assert got.is_cuda and got.is_contiguous()
    want = AR.to_chw(z[f"{name}_out"].astype(np.float32) / np.float32(255))
    assert _equal(got[0], want), f"{name}: {int((got[0].cpu().numpy() != want).sum())} of {want.size} values differ from PIL's"


@pytest.mark.parametrize("mode", AR.BLUR_MODES)
@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (7, 1), (2, 2)])
def test_blur_where_the_reflection_folds(env, mode, shape):
    _, ops = env
    img = np.ascontiguousarray(blocks_image()[5:5 + shape[0], 9:9 + shape[1]])
    k = AR.motion_kernel(mode, 3)
    got = ops.augment_views(_d(img[None]), [((), k)])
    assert _equal(got[0], AR.augment(img, (), k))


@pytest.mark.parametrize("mode", AR.BLUR_MODES)
@pytest.mark.parametrize("crop", [None, (0, 0, 131, 70), (40, 17, 70, 30), (63, 15, 3, 2)], ids=["whole", "borders", "interior", "seam"])
def test_blur_over_several_workgroups(env, mode, crop):
    """whole / borders: the window touches all four borders; interior: its halo comes from the image, not from a reflection;
    seam: a window across the tile corner of the whole image's grid, with its own grid of one."""
    _, ops = env
    got = ops.augment_views(_d(blocks_image()[None]), [((), AR.motion_kernel(mode, 3))], crop=crop)
    x0, y0, cw, ch = crop or (0, 0, 131, 70)
    want = AR.to_chw(blocks_blurred(mode)[y0:y0 + ch, x0:x0 + cw])
    assert _equal(got[0], want)
    if crop == (40, 17, 70, 30):                                      # (a reflection at the window's border would differ)
        inner = AR.to_chw(AR.blur32(AR.unit(blocks_image()[17:47, 40:110]), AR.motion_kernel(mode, 3)))
        assert not np.array_equal(inner, want)


def test_a_general_kernel_sums_in_row_major_order(env):
    """Nine live taps, some negative: the order of the fp32 sums shows."""
    _, ops = env
    k = np.array([[0.11, -0.07, 0.23], [0.05, 0.31, -0.13], [0.17, 0.09, 0.24]], dtype=np.float32)
    got = ops.augment_views(_d(blocks_image()[None]), [((), k)], crop=(0, 0, 131, 20))
    assert _equal(got[0], AR.to_chw(AR.blur32(AR.unit(blocks_image()), k)[:20]))


def test_three_views_three_records(env):
    """1961 pixels a view: the sum launch reads view 0 by words with one pixel left over, and view 2, which starts on an odd
    address, byte by byte."""
    _, ops = env
    imgs = np.stack([AR.random_image(37, 53, seed=s) for s in (1, 2, 3)])
    recs = [([("contrast", 1.21), ("brightness", 0.93)], AR.motion_kernel("diag_up", 3)), None,
            ([("brightness", 1.1), ("contrast", 0.7)], AR.motion_kernel("v", 3))]
    got = ops.augment_views(_d(imgs), recs, crop=(3, 2, 45, 30))
    assert tuple(got.shape) == (3, 3, 30, 45)
    assert _equal(got[1], AR.to_chw(AR.unit(imgs[1]))[:, 2:32, 3:48])                      # the empty record: lut[v]
    for v in range(3):
        steps, k = recs[v] or ((), None)
        assert _equal(got[v], AR.augment(imgs[v], steps, k, crop=(3, 2, 45, 30)))
        single = ops.augment_views(_d(imgs[v][None]), [recs[v]], crop=(3, 2, 45, 30))
        assert torch.equal(single[0].view(torch.int32), got[v].view(torch.int32))


@pytest.mark.parametrize("order", [("brightness", "contrast"), ("contrast", "brightness")])
def test_jitter_blur_window_chained(env, order):
    """Contrast's mean belongs to the whole 37 x 53 image while the window is 8 x 8: a mean over the window fails."""
    from wild_deep_mvs_amd.data import views
    _, ops = env
    img = AR.random_image(37, 53, seed=12)
    img[10:18, 20:28] = img[10:18, 20:28] // 4                        # the window is darker than the image
    a = views.ViewAugmentation(order=order, brightness=1.15, contrast=0.55, blur_mode="diag_down", ksize=3)
    crop = (20, 10, 8, 8)
    got = ops.augment_views(_d(img[None]), [a], crop=crop)
    assert _equal(got[0], AR.augment(img, a.steps(), a.blur_kernel(), crop=crop))
    window_only = AR.augment(np.ascontiguousarray(img[10:18, 20:28]), a.steps(), a.blur_kernel())
    assert not np.array_equal(window_only, got[0].cpu().numpy())


@pytest.mark.parametrize("rows", [4112, 4128])
def test_the_sum_of_l_needs_64_bits(env, rows):
    """An all-255 image of rows x 4096 with contrast 0.5 and an 8 x 8 window: m = 255, so every byte stays 255.  4112 rows: the sum
    of L is 2^32 - 65536, past a signed 32-bit word, and 2 S + n is past an unsigned one; 4128 rows: the sum itself is past
    2^32, where a wrapped sum gives m = 1 and bytes of 128."""
    _, ops = env
    S = rows * 4096 * 255
    assert S > 2 ** 31 and 2 * S + rows * 4096 > 2 ** 32 and (rows == 4112 or S > 2 ** 32)
    img = torch.full((1, rows, 4096, 3), 255, dtype=torch.uint8, device="cuda")
    got = ops.augment_views(img, [([("contrast", 0.5)], None)], crop=(2044, rows - 9, 8, 8))
    assert _equal(got[0], np.ones((3, 8, 8), dtype=np.float32))


def test_prepare_view_with_and_without_augment(env):
    """96 x 128 resized for a 64 x 64 window: resize -> augmentation of the WHOLE resized image -> crop; without ``augment`` the
    present path, bit for bit."""
    from wild_deep_mvs_amd.data import views
    _, ops = env
    img = LR.random_image(96, 128, 3, seed=6)
    K = np.array([[100.0, 0.0, 64.0], [0.0, 100.0, 48.0], [0.0, 0.0, 1.0]], dtype=np.float32)
    a = views.ViewAugmentation(order=("contrast", "brightness"), brightness=0.88, contrast=1.37, blur_mode="h", ksize=3)
    r, (rw, rh), (x0, y0, cw, ch) = LR.view_geometry(128, 96, "train", 64, 64)
    assert (rw, rh) == (85, 64) and (x0, y0, cw, ch) == (10, 0, 64, 64)
    whole = LR.resize(img, (rw, rh))
    im, new_K, got_r, d, m = views.prepare_view(_d(img), K, "train", 64, 64, augment=a)
    assert _equal(im, AR.augment(whole, a.steps(), a.blur_kernel(), crop=(x0, y0, cw, ch)))
    plain = views.prepare_view(_d(img), K, "train", 64, 64)
    want_im, want_K, want_r, _, _ = LR.prepare_view(img, K, "train", 64, 64)
    assert _equal(plain[0], want_im) and plain[1].tobytes() == want_K.tobytes() == new_K.tobytes() and plain[2] == want_r == got_r
    assert d is None and m is None
    same = views.prepare_view(_d(img), K, "train", 64, 64, augment=views.ViewAugmentation())      # nothing drawn: lut[v]
    assert _equal(same[0], want_im)
    with pytest.raises(ValueError):
        views.prepare_view(_d(img), K, "test", augment=a)


def test_two_runs_give_identical_bits(env):
    _, ops = env
    dev = _d(np.stack([blocks_image(), blocks_image()[::-1]]))
    recs = [([("brightness", 0.9), ("contrast", 1.4)], AR.motion_kernel("h", 3)), ([("contrast", 0.4)], AR.motion_kernel("diag_up", 3))]
    a = ops.augment_views(dev, recs, crop=(1, 1, 129, 68))
    b = ops.augment_views(dev, recs, crop=(1, 1, 129, 68))
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_argument_errors(env):
    import ctypes as C
    L, ops = env
    img = _d(blocks_image()[None])
    with pytest.raises(ValueError):
        ops.augment_views(img.cpu(), [None])
    with pytest.raises(ValueError):
        ops.augment_views(img.to(torch.float32), [None])
    with pytest.raises(ValueError):
        ops.augment_views(img[0], [None])
    with pytest.raises(ValueError):
        ops.augment_views(img[:, :, ::2], [None])
    with pytest.raises(ValueError):
        ops.augment_views(img, [None], crop=(100, 0, 32, 8))
    with pytest.raises(ValueError):
        ops.augment_views(img, [([("contrast", 0.5), ("contrast", 0.6)], None)])
    with pytest.raises(ValueError):
        ops.augment_views(img, [([("hue", 0.5)], None)])
    with pytest.raises(ValueError):
        ops.augment_views(img, [([("contrast", float("nan"))], None)])
    with pytest.raises(ValueError):
        ops.augment_views(img, [((), np.full((3, 3), np.inf))])
    # the C ABI checks for itself
    lib = L.lib()
    err = lambda: lib.pscv_last_error().decode()
    out = torch.empty((1, 3, 70, 131), dtype=torch.float32, device="cuda")
    ws = torch.zeros((1,), dtype=torch.int64, device="cuda")
    lut = ops._unit_table(img.device)
    w = (C.c_float * 9)(0, 0, 0, 0, 1, 0, 0, 0, 0)
    fac = (C.c_float * 2)(0.5, 1.5)

    def apply(V=1, o=(L.AUG_BRIGHTNESS, L.AUG_NONE), f=fac, k=w, win=(0, 0, 131, 70), wsp=ws):
        return lib.pscv_augment_apply(img.data_ptr(), V, 70, 131, (C.c_int * 2)(*o), f, k, wsp.data_ptr() if wsp is not None else None,
                                      *win, lut.data_ptr(), out.data_ptr(), None)

    assert apply(V=0) != 0 and "V=0" in err()
    assert apply(V=L.AUG_MAX_VIEWS + 1) != 0 and "V=" in err()
    assert apply(win=(0, 0, 132, 70)) != 0 and "window" in err()
    assert apply(win=(0, 69, 131, 2)) != 0 and "window" in err()
    assert apply(o=(L.AUG_CONTRAST, L.AUG_CONTRAST)) != 0 and "twice" in err()
    assert apply(f=(C.c_float * 2)(float("inf"), 1.0)) != 0 and "factors[0][0]" in err()
    assert apply(k=(C.c_float * 9)(0, 0, 0, 0, float("nan"), 0, 0, 0, 0)) != 0 and "weights[0][4]" in err()
    assert apply(o=(L.AUG_CONTRAST, L.AUG_NONE), wsp=None) != 0 and "workspace" in err()
    rc = lib.pscv_augment_grey_sums(img.data_ptr(), 1, 70, 131, (C.c_int * 2)(L.AUG_CONTRAST, L.AUG_NONE), fac, None, None)
    assert rc != 0 and "workspace" in err()
    assert apply() == 0                                               # and a good call goes through
    torch.cuda.synchronize()
    assert _equal(out[0], AR.augment(blocks_image(), [("brightness", 0.5)]))
