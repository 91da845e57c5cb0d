"""One view of a training or test sample, from the decoded image to the network's input: what the
reference's ``MVSDataset.read_img`` (after decoding, without ``data_augment``), ``rescale_calib``, ``center_crop``, the
``transpose([2, 0, 1])`` of ``data/md_yao.py:120`` and the depth lines of ``data/md_yao.py:99-102,123`` produce together.

  train   r = min(w / width, h / height); the image is resized to (int(w / r), int(h / r)) with PIL's Lanczos filter and the
          centre window of height x width is kept, from ((h' - height) // 2, (w' - width) // 2).  ``resize=False`` (the datasets
          whose images already have their size) keeps r = 1 and only crops.
  test    no resize; the window from (0, 0) whose sides are the largest multiples of ``multi``.
K follows in float32, as the reference's numpy products do: rows 0 and 1 times 1 / r, then the principal point moved by the window.
The ground-truth depth (train mode only) is resized to the resized image by nearest neighbour and cut to the same window; its mask
is (depth >= min_d) & (depth < max_d).

The pixels never leave the GPU: ``ops.resize_lanczos_u8`` computes the window only and writes the fp32 [3,h,w] image beside the
bytes; ``ops.depth_nearest_crop`` does the depth.  K is nine numbers and stays on the host.  Decoding the file and the random
``data_augmentation`` are the caller's (out of scope, section 2k).  There is no CPU path."""
from __future__ import annotations

import numpy as np
import torch

from .. import ops

MODES = ("train", "test")


def view_geometry(w, h, mode, height=512, width=512, multi=32, resize=True):
    """-> (r, (w', h') of the resized image, (x0, y0, cw, ch) of the window kept) for a w x h image."""
    if mode not in MODES:
        raise ValueError(f"prepare_view: mode '{mode}' must be one of {MODES}")
    if mode == "test":
        cw, ch = (w // multi) * multi, (h // multi) * multi
        if cw < 1 or ch < 1:
            raise ValueError(f"prepare_view: a {w} x {h} image holds no multiple of {multi}")
        return 1, (w, h), (0, 0, cw, ch)
    r = min(w / width, h / height) if resize else 1
    rw, rh = (int(w / r), int(h / r)) if resize else (w, h)
    if rw < width or rh < height:
        # (the reference would slice from a negative index here and return a window of another size)
        raise ValueError(f"prepare_view: the {rw} x {rh} image is smaller than the {width} x {height} window")
    return r, (rw, rh), ((rw - width) // 2, (rh - height) // 2, width, height)


def rescale_calib(r, K):
    """K fp32 [3,3] with rows 0 and 1 scaled by 1 / r (a float32 matrix product, as the reference's)."""
    m = np.eye(3, dtype=np.float32)
    m[0, 0] = m[1, 1] = 1 / r
    return m @ np.asarray(K, dtype=np.float32)


def crop_calib(x0, y0, K):
    """K fp32 [3,3] of the window that starts at column x0, row y0."""
    m = np.eye(3, dtype=np.float32)
    m[0, 2], m[1, 2] = -x0, -y0
    return m @ np.asarray(K, dtype=np.float32)


def prepare_view(img_u8: torch.Tensor, K, mode: str, height: int = 512, width: int = 512, multi: int = 32, resize: bool = True,
                 depth: torch.Tensor = None, depth_range=None):
    """img_u8 uint8 [H,W,3] on the GPU (the decoded file), K [3,3] (numpy or tensor, any device) ->
    (im fp32 [3,h,w] on the GPU in [0,1], new_K fp32 [3,3] numpy, r, depth, mask).
    ``depth`` fp32 [th,tw] on the GPU with ``depth_range`` = (min_d, max_d), train mode only, gives depth fp32 [h,w] and mask bool
    [h,w] on the GPU; both are None without it."""
    if img_u8.dim() != 3 or img_u8.shape[2] != 3:
        raise ValueError(f"prepare_view: uint8 [H,W,3] expected, got {tuple(img_u8.shape)}")
    H, W = int(img_u8.shape[0]), int(img_u8.shape[1])
    r, (rw, rh), (x0, y0, cw, ch) = view_geometry(W, H, mode, height, width, multi, resize)
    _, im = ops.resize_lanczos_u8(img_u8, (rw, rh), crop=(x0, y0, cw, ch), want_f32=True)
    K = K.detach().cpu().numpy() if isinstance(K, torch.Tensor) else K
    new_K = crop_calib(x0, y0, rescale_calib(r, K))
    d = mask = None
    if depth is not None:
        if mode != "train":
            raise ValueError("prepare_view: the reference resizes a ground-truth depth in train mode only")
        if depth_range is None:
            raise ValueError("prepare_view: depth needs depth_range = (min_d, max_d) for its mask")
        d, mask = ops.depth_nearest_crop(depth, (rh, rw), crop=(y0, x0, ch, cw), min_d=depth_range[0], max_d=depth_range[1])
        mask = mask.view(torch.bool)
    return im, new_K, r, d, mask
