"""Numpy restatement of the image preparation (csrc/image_resample.hip, wild_deep_mvs_amd/data/views.py):
PIL's ``Image.resize(size, resample=Image.LANCZOS)`` on 8-bit images, the nearest-neighbour index of ``F.interpolate`` on CPU
torch, and what the reference's ``read_img`` + ``rescale_calib`` + ``center_crop`` make of one view.

PIL's resampling (libImaging/Resample.c) is deterministic: per axis a table of float64 Lanczos weights, normalised per output
sample and rounded to 22-bit fixed point; an int32 accumulator that starts at 2^21, is shifted right by 22 and clamped to
[0, 255]; the horizontal pass first, its result ROUNDED TO 8 BITS, then the vertical pass; a pass whose length does not change is
skipped.  Everything here is written scalar and slow on purpose: it is the yardstick, not the implementation.  ``math.sin`` (libm,
what PIL calls), not ``numpy.sin``.
PIL forms the filter argument as ``(k + first - center + 0.5) * (1.0 / fs)``: the product with the reciprocal, not a division."""
from __future__ import annotations

import math

import numpy as np

PRECISION_BITS = 32 - 8 - 2


def sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def lanczos(x):
    return sinc(x) * sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


def tables(in_len, out_len):
    """-> (coeff int64 [out_len, ksize], bounds int64 [out_len, 2] = (first, n), ksize).  Entries past n are 0."""
    scale = in_len / out_len
    fs = max(scale, 1.0)
    support = 3.0 * fs
    ksize = 2 * int(math.ceil(support)) + 1
    ss = 1.0 / fs
    coeff = np.zeros((out_len, ksize), dtype=np.int64)
    bounds = np.zeros((out_len, 2), dtype=np.int64)
    for o in range(out_len):
        center = (o + 0.5) * scale
        first = max(int(center - support + 0.5), 0)
        last = min(int(center + support + 0.5), in_len)
        n = last - first
        w = [lanczos((k + first - center + 0.5) * ss) for k in range(n)]
        total = 0.0
        for v in w:
            total += v
        if total != 0.0:
            w = [v / total for v in w]
        for k, v in enumerate(w):
            coeff[o, k] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        bounds[o] = (first, n)
    return coeff, bounds, ksize


def resample_pass(img, out_len, axis):
    """One pass over uint8 ``img`` [H, W] or [H, W, C] along ``axis`` (0 = rows change, the vertical pass; 1 = the horizontal)."""
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    coeff, bounds, _ = tables(src.shape[0], out_len)
    out = np.empty((out_len,) + src.shape[1:], dtype=np.uint8)
    for o in range(out_len):
        first, n = bounds[o]
        acc = (1 << (PRECISION_BITS - 1)) + np.tensordot(coeff[o, :n], src[first:first + n], axes=(0, 0))
        assert np.abs(acc).max() < 2 ** 31                       # PIL's accumulator is an int32
        out[o] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize(img, size):
    """PIL's ``Image.fromarray(img).resize(size, resample=Image.LANCZOS)`` as an array; ``size`` = (width, height)."""
    w, h = size
    tmp = resample_pass(img, w, 1) if w != img.shape[1] else img
    return resample_pass(tmp, h, 0) if h != img.shape[0] else tmp


def to_f32_chw(img):
    """What ``np.array(pil, dtype=np.float32) / 255.`` followed by ``transpose([2, 0, 1])`` holds."""
    if img.ndim == 2:
        img = img[:, :, None]
    return np.ascontiguousarray((img.astype(np.float32) / np.float32(255)).transpose(2, 0, 1))


def nearest_index(out_len, in_len):
    """Source index of every output index of ``F.interpolate(mode="nearest")`` on CPU torch: fp32 scale, fp32 product, floor."""
    scale = np.float32(in_len) / np.float32(out_len)
    dst = np.arange(out_len, dtype=np.float32)
    return np.minimum(np.floor(dst * scale).astype(np.int64), in_len - 1)


def depth_nearest_crop(depth, size_hw, crop, min_d, max_d):
    """depth fp32 [th, tw] -> nearest resize to ``size_hw`` = (oh, ow), window ``crop`` = (y0, x0, ch, cw); mask = (d >= min_d) &
    (d < max_d) with the bounds rounded to fp32, as torch compares an fp32 tensor with a Python number."""
    oh, ow = size_hw
    y0, x0, ch, cw = crop
    iy, ix = nearest_index(oh, depth.shape[0])[y0:y0 + ch], nearest_index(ow, depth.shape[1])[x0:x0 + cw]
    d = np.ascontiguousarray(depth[iy][:, ix])
    return d, ((d >= np.float32(min_d)) & (d < np.float32(max_d))).astype(np.uint8)


def view_geometry(w, h, mode, height=512, width=512, multi=32, do_resize=True):
    """-> (ratio r, resized (w', h'), crop (x0, y0, cw, ch)) of one view of a w x h image."""
    if mode == "train":
        r = min(w / width, h / height) if do_resize else 1
        rw, rh = (int(w / r), int(h / r)) if do_resize else (w, h)
        return r, (rw, rh), ((rw - width) // 2, (rh - height) // 2, width, height)
    return 1, (w, h), (0, 0, (w // multi) * multi, (h // multi) * multi)


def calib(K, r, x0, y0):
    """K's rows 0 and 1 times 1 / r, then the principal point moved by the crop, as float32 matrix products."""
    s = np.eye(3, dtype=np.float32)
    s[0, 0] = s[1, 1] = 1 / r
    c = np.eye(3, dtype=np.float32)
    c[0, 2], c[1, 2] = -x0, -y0
    return c @ (s @ np.asarray(K, dtype=np.float32))


def prepare_view(img, K, mode, height=512, width=512, multi=32, do_resize=True, depth=None, depth_range=None):
    """-> (im fp32 [3, h, w], new_K fp32 [3, 3], r, depth or None, mask or None) of one decoded view ``img`` uint8 [H, W, 3]."""
    H, W = img.shape[:2]
    r, (rw, rh), (x0, y0, cw, ch) = view_geometry(W, H, mode, height, width, multi, do_resize)
    res = resize(img, (rw, rh))[y0:y0 + ch, x0:x0 + cw]
    d = m = None
    if depth is not None:
        d, m = depth_nearest_crop(depth, (rh, rw), (y0, x0, ch, cw), *depth_range)
    return to_f32_chw(res), calib(K, r, x0, y0), r, d, m


def resized_size(size, min_size):
    """(width, height) of preprocess.py's getResizedSize."""
    w, h = size
    ratio = min(w / min_size, h / min_size)
    return int(w / ratio / 32) * 32, int(h / ratio / 32) * 32


def block_image(h, w, c, cell=5, seed=0):
    """0 / 255 blocks of ``cell`` pixels: step edges, so that the Lanczos overshoot reaches both clamps."""
    rng = np.random.default_rng(seed)
    blocks = rng.integers(0, 2, ((h + cell - 1) // cell, (w + cell - 1) // cell, c), dtype=np.uint8) * np.uint8(255)
    return np.ascontiguousarray(np.repeat(np.repeat(blocks, cell, axis=0), cell, axis=1)[:h, :w])


def random_image(h, w, c=3, seed=0):
    """Smooth gradient plus noise plus a few saturated blocks; [h, w] for c = 0."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h, w, max(c, 1)), dtype=np.uint8)
    img[h // 4:h // 2, w // 3:w // 2] = 255
    img[h // 2:h // 2 + max(h // 8, 1), : w // 2] = 0
    return np.ascontiguousarray(img[:, :, 0] if c == 0 else img)
