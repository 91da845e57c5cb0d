"""CPU: the host side of the training-view augmentation.  The numpy restatement tests/_augment_ref.py is
the yardstick of the GPU tests, so it is held here against PIL's own ``ImageEnhance`` where PIL is installed (zero differing bytes
over 240 random images and factors) and against the fixture tests/golden/augment_tiny.npz (PIL's outputs, recorded); the blur's
fp32 rule against float64; ``data.views.ViewAugmentation`` / ``draw_augmentation`` against the reference's kernel construction and
its two numpy draws; and the argument checks that need no device."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import _augment_ref as AR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ("bright", "bright_hi", "contrast", "clip", "bc", "cb", "half")
NAMES = {1: "brightness", 2: "contrast"}


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(os.path.join(GOLDEN, "augment_tiny.npz")))


def case_steps(z, name):
    return [(NAMES[int(o)], float(f)) for o, f in zip(z[f"{name}_ops"], z[f"{name}_factors"])]


def live_cases():
    """240 (image, steps): factors inside [0, 1], on both sides of it, exactly 0 and 1, single steps and both chained orders, noisy
    and posterised images."""
    rng = np.random.default_rng(11)
    special = [1.0, 0.0, -0.25, 1.5, 0.3, 1.0 + 50 / 255, 1.0 - 50 / 255, 2.75]
    out = []
    for k in range(240):
        h, w = int(rng.integers(1, 20)), int(rng.integers(1, 24))
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        if k % 5 == 0:
            img = (img // 64 * 85).astype(np.uint8)                  # posterised: 0, 85, 170, 255
        f = [float(np.float32(special[k % len(special)] if k % 3 == 0 else rng.uniform(-0.5, 2.0))),
             float(np.float32(special[(k // 3) % len(special)] if k % 4 == 0 else rng.uniform(0.0, 1.6)))]
        kind = k % 4
        steps = [[("brightness", f[0])], [("contrast", f[0])], [("brightness", f[0]), ("contrast", f[1])],
                 [("contrast", f[0]), ("brightness", f[1])]][kind]
        out.append((img, steps))
    return out


def test_restatement_equals_live_pil():
    pytest.importorskip("PIL")
    from PIL import Image, ImageEnhance
    cases = live_cases()
    factors = [f for _, steps in cases for _, f in steps]
    assert len(cases) >= 200 and 1.0 in factors and min(factors) < 0 and max(factors) > 1 and any(0 < f < 1 for f in factors)
    assert {tuple(n for n, _ in steps) for _, steps in cases} >= {("brightness", "contrast"), ("contrast", "brightness")}
    differing = 0
    for img, steps in cases:
        pil = Image.fromarray(img)
        for name, f in steps:
            pil = (ImageEnhance.Brightness if name == "brightness" else ImageEnhance.Contrast)(pil).enhance(f)
        differing += int((AR.jitter(img, steps) != np.asarray(pil)).sum())
    assert differing == 0


def test_grey_is_pils_convert_l():
    pytest.importorskip("PIL")
    from PIL import Image, ImageStat
    img = AR.random_image(17, 23, seed=3)
    pil = Image.fromarray(img).convert("L")
    assert np.array_equal(AR.grey(img), np.asarray(pil))
    assert AR.grey_mean(img) == int(ImageStat.Stat(pil).mean[0] + 0.5)


@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_the_fixture(name):
    z = fixture()
    got = AR.jitter(z[f"{name}_in"], case_steps(z, name))
    assert got.dtype == np.uint8 and np.array_equal(got, z[f"{name}_out"])


def test_the_fixture_bites():
    z = fixture()
    assert (z["clip_out"] == 0).any() and (z["clip_out"] == 255).any() and float(z["clip_factors"][0]) > 1
    L = AR.grey(z["half_in"]).astype(np.int64)
    assert (2 * int(L.sum())) % (2 * L.size) == L.size                # the mean is x.5 exactly
    assert AR.grey_mean(z["half_in"]) == int(L.sum()) // L.size + 1
    assert z["bc_ops"].tolist() == [1, 2] and z["cb_ops"].tolist() == [2, 1]
    for name in CASES:                                                # rounding to nearest instead of truncating would differ
        img = z[f"{name}_in"]
        (op, f) = case_steps(z, name)[0]
        t = AR.blend_t(0 if op == "brightness" else AR.grey_mean(img), img, f)
        assert ((t > 0) & (t < 255) & (np.floor(t) != np.rint(t))).any(), name


@pytest.mark.parametrize("mode", AR.BLUR_MODES)
def test_fp32_blur_is_within_2_to_the_minus_22_of_float64(mode):
    """The weights, three products and two sums are each rounded to half an ulp on magnitudes of at most 1: 4 x 2^-24."""
    x = AR.unit(AR.random_image(19, 27, seed=5))
    for shape in [(19, 27), (1, 1), (1, 7), (7, 1), (2, 2)]:
        part = np.ascontiguousarray(x[:shape[0], :shape[1]])
        got = AR.blur32(part, AR.motion_kernel(mode, 3))
        want = AR.blur64(part, AR.embed3(AR.motion_kernel64(mode, 3)))
        assert got.dtype == np.float32 and np.abs(got.astype(np.float64) - want).max() <= 2.0 ** -22


@pytest.mark.parametrize("mode", AR.BLUR_MODES)
def test_ksize_1_is_the_identity_bitwise(mode):
    x = AR.unit(np.arange(256 * 3, dtype=np.int64).reshape(16, 16, 3).astype(np.uint8))
    k = AR.motion_kernel(mode, 1)
    assert k.tolist() == [[0, 0, 0], [0, 1, 0], [0, 0, 0]]
    assert AR.blur32(x, k).tobytes() == x.tobytes()


def test_reflect101():
    assert [AR.reflect101(i, 5) for i in (-1, 0, 4, 5)] == [1, 0, 4, 3]
    assert [AR.reflect101(i, 2) for i in (-1, 0, 1, 2)] == [1, 0, 1, 0]
    assert [AR.reflect101(i, 1) for i in (-1, 0, 1)] == [0, 0, 0]


def test_the_four_kernels():
    from wild_deep_mvs_amd.data import views
    e = np.exp(-1.0 / (2.0 * 9.0 / 16.0))
    h = np.array([[0, 0, 0], [e, 1, e], [0, 0, 0]]) / (1 + 2 * e)
    assert np.allclose(AR.motion_kernel64("h", 3), h, rtol=0, atol=1e-15)
    masks = {"h": np.array([[0, 0, 0], [1, 1, 1], [0, 0, 0]]), "v": np.array([[0, 1, 0], [0, 1, 0], [0, 1, 0]]),
             "diag_down": np.eye(3), "diag_up": np.eye(3)[::-1]}
    for mode in AR.BLUR_MODES:
        for ksize in (1, 3):
            k64 = AR.motion_kernel64(mode, ksize)
            assert abs(k64.sum() - 1.0) <= 1e-15
            got = views.ViewAugmentation(blur_mode=mode, ksize=ksize).blur_kernel()
            assert got.dtype == np.float32 and got.shape == (3, 3) and got.tobytes() == AR.motion_kernel(mode, ksize).tobytes()
            assert abs(float(got.astype(np.float64).sum()) - 1.0) <= 4 * 2.0 ** -24
        assert np.array_equal(AR.motion_kernel64(mode, 3) != 0, masks[mode] != 0)
    assert views.ViewAugmentation(blur_mode="h", ksize=3).blur_kernel().tobytes() == h.astype(np.float32).tobytes()


def test_draw_augmentation_follows_the_references_draws():
    from wild_deep_mvs_amd.data import views
    orders, ksizes, modes = set(), set(), set()
    for s in range(200):
        np.random.seed(s)
        want = AR.draw_blur()
        np.random.seed(s)
        torch.manual_seed(s)
        a = views.draw_augmentation()
        assert (a.blur_mode, a.ksize) == want
        assert 1 - 50 / 255 - 1e-6 <= a.brightness <= 1 + 50 / 255 + 1e-6 and 0.3 - 1e-6 <= a.contrast <= 1.5 + 1e-6
        assert [n for n, _ in a.steps()] == list(a.order)
        orders.add(a.order)
        ksizes.add(a.ksize)
        modes.add(a.blur_mode)
    assert orders == {("brightness", "contrast"), ("contrast", "brightness")}
    assert ksizes == {1, 3} and modes == set(AR.BLUR_MODES)
    # torch's generator: randperm(4), then the two factors
    torch.manual_seed(5)
    perm = torch.randperm(4).tolist()
    b = float(torch.empty(1).uniform_(*views.JITTER_BRIGHTNESS))
    c = float(torch.empty(1).uniform_(*views.JITTER_CONTRAST))
    torch.manual_seed(5)
    a = views.draw_augmentation()
    assert (a.brightness, a.contrast) == (b, c) and a.order == tuple(("brightness", "contrast")[i] for i in perm if i < 2)


def test_view_augmentation_records():
    from wild_deep_mvs_amd.data import views
    a = views.ViewAugmentation(order=("contrast", "brightness"), contrast=0.5, blur_mode="v", ksize=3)
    steps, kernel = a.record()
    assert steps == [("contrast", 0.5)] and kernel.tobytes() == AR.motion_kernel("v", 3).tobytes()
    assert views.ViewAugmentation().record()[0] == []
    for bad in (dict(order=("contrast",)), dict(blur_mode="x"), dict(ksize=5), dict(order=("contrast", "contrast"))):
        with pytest.raises(ValueError):
            views.ViewAugmentation(**bad)


def test_augment_views_rejects_bad_arguments_without_a_device():
    from wild_deep_mvs_amd import ops
    img = torch.zeros((1, 6, 7, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match="GPU"):
        ops.augment_views(img, [None])                                 # a CPU tensor
    with pytest.raises(ValueError, match="uint8"):
        ops.augment_views(img.float(), [None])
    for bad in (img[0], torch.zeros((1, 6, 7, 4), dtype=torch.uint8), torch.zeros((1, 0, 7, 3), dtype=torch.uint8)):
        with pytest.raises(ValueError, match="expected"):
            ops.augment_views(bad, [None])
    with pytest.raises(ValueError, match="contiguous"):
        ops.augment_views(torch.zeros((1, 6, 14, 3), dtype=torch.uint8)[:, :, ::2], [None])
    with pytest.raises(ValueError, match="records"):
        ops.augment_views(img, [None, None])
    for crop in [(-1, 0, 4, 4), (0, -1, 4, 4), (4, 0, 4, 4), (0, 3, 4, 4), (0, 0, 0, 4), (0, 0, 4, 0), (0, 0, 8, 4)]:
        with pytest.raises(ValueError, match="outside"):
            ops.augment_views(img, [None], crop=crop)
    with pytest.raises(ValueError, match="at most"):
        ops.augment_views(torch.zeros((17, 2, 2, 3), dtype=torch.uint8), [None] * 17)


def test_prepare_view_augments_in_train_mode_only():
    from wild_deep_mvs_amd.data import views
    img = torch.zeros((64, 96, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match="train mode"):
        views.prepare_view(img, np.eye(3), "test", augment=views.ViewAugmentation(brightness=0.9))


def test_the_abi_checks_its_records():
    """Host-side argument checks of the C ABI: nothing is launched, no pointer is followed on the device."""
    import ctypes as C
    from wild_deep_mvs_amd import _lib as L
    lib = L.lib()
    err = lambda: lib.pscv_last_error().decode()
    assert L.AUG_MAX_VIEWS >= 16 and (L.AUG_NONE, L.AUG_BRIGHTNESS, L.AUG_CONTRAST) == (0, 1, 2)
    assert lib.pscv_augment_workspace(5) == 40
    assert lib.pscv_augment_workspace(0) < 0 and "V=0" in err()
    assert lib.pscv_augment_workspace(L.AUG_MAX_VIEWS + 1) < 0 and f"V={L.AUG_MAX_VIEWS + 1}" in err()
    ops1, fac1 = (C.c_int * 2)(L.AUG_BRIGHTNESS, L.AUG_NONE), (C.c_float * 2)(0.9, 1.0)
    w1 = (C.c_float * 9)(0, 0, 0, 0, 1, 0, 0, 0, 0)
    fake = 4096                                                        # stands for device memory; every call fails before a launch

    def apply(V=1, H=6, W=7, ops=ops1, fac=fac1, w=w1, ws=None, win=(0, 0, 7, 6), imgs=fake):
        return lib.pscv_augment_apply(imgs, V, H, W, ops, fac, w, ws, *win, fake, fake, None)

    assert apply(V=0) != 0 and "V=0" in err()
    assert apply(V=17) != 0 and "V=17" in err()
    assert apply(imgs=None) != 0 and "imgs" in err()
    assert apply(H=0) != 0 and "image" in err()
    for win in [(-1, 0, 4, 4), (0, 0, 8, 6), (0, 0, 7, 7), (6, 0, 2, 1), (0, 0, 0, 1)]:
        assert apply(win=win) != 0 and "window" in err() and "outside" in err()
    assert apply(ops=(C.c_int * 2)(L.AUG_BRIGHTNESS, L.AUG_BRIGHTNESS)) != 0 and "twice" in err()
    assert apply(ops=(C.c_int * 2)(3, 0)) != 0 and "ops[0][0]" in err()
    for bad in (float("nan"), float("inf")):
        assert apply(fac=(C.c_float * 2)(bad, 1.0)) != 0 and "factors[0][0]" in err()
        assert apply(w=(C.c_float * 9)(0, 0, bad, 0, 1, 0, 0, 0, 0)) != 0 and "weights[0][2]" in err()
    assert apply(ops=(C.c_int * 2)(L.AUG_CONTRAST, L.AUG_NONE)) != 0 and "workspace" in err()
    assert apply(w=None) != 0 and "weights" in err()
    sums = lambda **kw: lib.pscv_augment_grey_sums(kw.get("imgs", fake), kw.get("V", 1), 6, 7, kw.get("ops", ops1), fac1, kw.get("ws"), None)
    assert sums() == 0                                                 # no contrast step: nothing to do, nothing launched
    assert sums(V=0) != 0 and "V=0" in err()
    assert sums(ops=(C.c_int * 2)(L.AUG_CONTRAST, L.AUG_NONE)) != 0 and "workspace" in err()
    assert sums(ops=(C.c_int * 2)(L.AUG_CONTRAST, L.AUG_CONTRAST)) != 0 and "twice" in err()
