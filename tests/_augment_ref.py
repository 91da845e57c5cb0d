"""Numpy restatement of the training-view augmentation (csrc/image_augment.hip,
wild_deep_mvs_amd/data/views.py): what the reference's ``MVSDataset.data_augmentation`` does to one 8-bit RGB image.

Colour jitter is torchvision's ``ColorJitter`` on the PIL image, that is ``ImageEnhance.Brightness`` and ``ImageEnhance.Contrast``,
that is ``Image.blend(degenerate, image, factor)`` (libImaging/Blend.c): per byte, in fp32, ``t = deg + a * (v - deg)`` with the
product rounded, then the sum; truncated for 0 <= a <= 1, clipped to [0, 255] and truncated otherwise.  Brightness blends with
black, contrast with the grey level ``int(mean(L) + 0.5)`` of the WHOLE image, L being PIL's ``convert("L")``.
The blur is ``cv2.filter2D`` with BORDER_REFLECT_101 on ``float32(v) / 255``; the engine's rule for it (weights rounded once to
fp32, zero taps skipped, the others summed in row-major order, every product and sum rounded to fp32) is ``blur32``, and
``blur64`` is the same correlation in float64.  Everything is written plainly and slowly: it is the yardstick.
tests/test_augment_cpu.py holds ``blend`` and the two enhancers against PIL itself."""
from __future__ import annotations

import numpy as np

BLUR_MODES = ["h", "v", "diag_down", "diag_up"]
MAX_KERNEL_SIZE = 3


def blend_t(deg, img, factor):
    """The fp32 value Blend.c forms per byte: deg + a * (v - deg), two roundings.  ``deg`` a byte value or an array like img."""
    a = np.float32(factor)
    diff = (img.astype(np.int32) - np.asarray(deg, dtype=np.int32)).astype(np.float32)
    prod = (a * diff).astype(np.float32)
    return (np.asarray(deg, dtype=np.int32).astype(np.float32) + prod).astype(np.float32)


def blend(deg, img, factor):
    """``Image.blend(degenerate, image, factor)`` on uint8 arrays."""
    a = np.float32(factor)
    t = blend_t(deg, img, factor)
    if a >= 0 and a <= 1:
        return t.astype(np.int32).astype(np.uint8)                      # (a C cast: truncation; t lies in [0, 255])
    return np.where(t <= 0, 0, np.where(t >= 255, 255, np.clip(t, 0, 255).astype(np.int32))).astype(np.uint8)


def grey(img):
    """PIL's ``convert("L")`` of an RGB image."""
    c = img.astype(np.int64)
    return ((19595 * c[..., 0] + 38470 * c[..., 1] + 7471 * c[..., 2] + 0x8000) >> 16).astype(np.uint8)


def grey_mean(img):
    """``int(ImageStat.Stat(img.convert("L")).mean[0] + 0.5)`` in integers: (2 S + n) // (2 n)."""
    L = grey(img)
    S, n = int(L.astype(np.int64).sum()), L.size
    return (2 * S + n) // (2 * n)


def brightness(img, factor):
    return blend(0, img, factor)


def contrast(img, factor):
    return blend(grey_mean(img), img, factor)


STEPS = {"brightness": brightness, "contrast": contrast}


def jitter(img, steps):
    """``steps`` = [(name, factor)] in the order they run."""
    for name, factor in steps:
        img = STEPS[name](img, factor)
    return img


def reflect101(i, n):
    """BORDER_REFLECT_101 for i in [-1, n]: -1 reads 1, n reads n - 2, an axis of length 1 reads 0."""
    if n == 1:
        return 0
    if i < 0:
        return -i
    if i >= n:
        return 2 * n - 2 - i
    return i


def unit(img):
    """``np.array(pil, dtype=np.float32) / 255.``"""
    return img.astype(np.float32) / np.float32(255)


def _taps(x, dtype):
    """x [H, W, C] -> the nine shifted copies tap[t][y, x] = x[reflect(y + t // 3 - 1), reflect(x + t % 3 - 1)]."""
    H, W = x.shape[:2]
    out = []
    for t in range(9):
        iy = [reflect101(y + t // 3 - 1, H) for y in range(H)]
        ix = [reflect101(c + t % 3 - 1, W) for c in range(W)]
        out.append(x[iy][:, ix].astype(dtype))
    return out


def blur32(x, kernel):
    """The engine's rule: x fp32 [H, W, C], kernel [3, 3] rounded once to fp32; taps of weight zero skipped, the others
    accumulated in row-major order, each product and each sum rounded to fp32.  -> fp32 [H, W, C]."""
    w = np.asarray(kernel, dtype=np.float32).reshape(9)
    acc = None
    for t, tap in enumerate(_taps(x.astype(np.float32), np.float32)):
        if w[t] == 0:
            continue
        prod = (w[t] * tap).astype(np.float32)
        acc = prod if acc is None else (acc + prod).astype(np.float32)
    return np.zeros(x.shape, dtype=np.float32) if acc is None else acc


def blur64(x, kernel):
    """The same correlation in float64 with the float64 kernel."""
    w = np.asarray(kernel, dtype=np.float64).reshape(9)
    acc = np.zeros(x.shape, dtype=np.float64)
    for t, tap in enumerate(_taps(x, np.float64)):
        acc += w[t] * tap
    return acc


def motion_kernel64(mode, ksize):
    """``motion_blur``'s kernel in float64, [ksize, ksize] (data/MVSDataset.py:129-143 in our words)."""
    c = int((ksize - 1) / 2)
    k = np.zeros((ksize, ksize))
    if mode == "h":
        k[c, :] = 1.0
    elif mode == "v":
        k[:, c] = 1.0
    elif mode == "diag_down":
        k = np.eye(ksize)
    elif mode == "diag_up":
        k = np.flip(np.eye(ksize), 0)
    else:
        raise ValueError(mode)
    var = ksize * ksize / 16.0
    g = np.repeat(np.arange(ksize)[:, np.newaxis], ksize, axis=-1)
    k = k * np.exp(-(np.square(g - c) + np.square(g.T - c)) / (2.0 * var))
    return k / np.sum(k)


def embed3(k):
    """A 1 x 1 or 3 x 3 kernel as [3, 3] float64 (the 1 x 1 kernel in the centre)."""
    out = np.zeros((3, 3))
    c = (3 - k.shape[0]) // 2
    out[c:3 - c, c:3 - c] = k
    return out


def motion_kernel(mode, ksize):
    """fp32 [3, 3]: what the kernel reads."""
    return embed3(motion_kernel64(mode, ksize)).astype(np.float32)


def draw_blur():
    """The reference's two numpy calls, in its order, on numpy's global generator -> (mode, ksize)."""
    mode = np.random.choice(BLUR_MODES)
    ksize = np.random.randint(0, (MAX_KERNEL_SIZE + 1) / 2) * 2 + 1
    return str(mode), int(ksize)


def to_chw(x):
    return np.ascontiguousarray(x.transpose(2, 0, 1))


def augment(img, steps=(), kernel=None, crop=None):
    """img uint8 [H, W, 3] -> fp32 [3, ch, cw]: jitter, /255, blur32 over the whole image, then the window (x0, y0, cw, ch)."""
    x = unit(jitter(img, steps))
    if kernel is not None:
        x = blur32(x, kernel)
    if crop is not None:
        x0, y0, cw, ch = crop
        x = x[y0:y0 + ch, x0:x0 + cw]
    return to_chw(x)


def random_image(h, w, seed=0):
    """Noise with a saturated and a black block and a smooth channel."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    img[h // 4:h // 2, w // 3:w // 2] = 255
    img[h // 2:h // 2 + max(h // 8, 1), : w // 2] = 0
    img[:, :, 1] = ((np.add.outer(np.arange(h), np.arange(w)) * 3) % 256).astype(np.uint8)
    return np.ascontiguousarray(img)
