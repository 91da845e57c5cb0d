"""One view of a training or test sample, from the decoded image to the network's input: what the
reference's ``MVSDataset.read_img`` (after decoding; ``data_augment`` through ``augment=``), ``rescale_calib``, ``center_crop``, the
``transpose([2, 0, 1])`` of ``data/md_yao.py:120`` and the depth lines of ``data/md_yao.py:99-102,123`` produce together.

  train   r = min(w / width, h / height); the image is resized to (int(w / r), int(h / r)) with PIL's Lanczos filter and the
          centre window of height x width is kept, from ((h' - height) // 2, (w' - width) // 2).  ``resize=False`` (the datasets
          whose images already have their size) keeps r = 1 and only crops.
  test    no resize; the window from (0, 0) whose sides are the largest multiples of ``multi``.
K follows in float32, as the reference's numpy products do: rows 0 and 1 times 1 / r, then the principal point moved by the window.
The ground-truth depth (train mode only) is resized to the resized image by nearest neighbour and cut to the same window; its mask
is (depth >= min_d) & (depth < max_d).

The pixels never leave the GPU: ``ops.resize_lanczos_u8`` computes the window only and writes the fp32 [3,h,w] image beside the
bytes; ``ops.depth_nearest_crop`` does the depth.  K is nine numbers and stays on the host.  Decoding the file is the caller's.

The random ``data_augmentation`` of BlendedMVS's training views (``data/MVSDataset.py:124-150``, section 2m) is ``augment=``:
``draw_augmentation()`` draws a ``ViewAugmentation`` with the reference's random calls, and ``prepare_view`` then resizes the
WHOLE image, because contrast's mean and the blur's borders are those of the whole image, and lets ``ops.augment_views`` compute
the window.  There is no CPU path."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from .. import ops

MODES = ("train", "test")
BLUR_MODES = ("h", "v", "diag_down", "diag_up")
# torchvision's ranges for ColorJitter(brightness=50/255, contrast=(0.3, 1.5)): [max(0, 1 - b), 1 + b] and the pair as given
JITTER_BRIGHTNESS = (max(0.0, 1 - 50 / 255), 1 + 50 / 255)
JITTER_CONTRAST = (0.3, 1.5)
MAX_BLUR_KSIZE = 3


@dataclass(frozen=True)
class ViewAugmentation:
    """One draw of the reference's ``data_augmentation``: the colour steps in ``order`` (a step whose factor is None is absent),
    then ``motion_blur`` with ``blur_mode`` and ``ksize`` (1 = no blur, or 3)."""
    order: Tuple[str, ...] = ("brightness", "contrast")
    brightness: Optional[float] = None
    contrast: Optional[float] = None
    blur_mode: str = "h"
    ksize: int = 1

    def __post_init__(self):
        if sorted(self.order) != ["brightness", "contrast"]:
            raise ValueError(f"ViewAugmentation: order {self.order} must hold 'brightness' and 'contrast' once each")
        if self.blur_mode not in BLUR_MODES:
            raise ValueError(f"ViewAugmentation: blur_mode '{self.blur_mode}' must be one of {BLUR_MODES}")
        if self.ksize not in (1, MAX_BLUR_KSIZE):
            raise ValueError(f"ViewAugmentation: ksize {self.ksize} must be 1 or {MAX_BLUR_KSIZE}")

    def steps(self):
        """[(name, factor)] of the steps that are present, in the order they run."""
        return [(name, getattr(self, name)) for name in self.order if getattr(self, name) is not None]

    def blur_kernel(self) -> np.ndarray:
        """``motion_blur``'s kernel, built in float64 as the reference builds it and cast to fp32 [3,3] (ksize 1: a centre of 1)."""
        k = self.ksize
        c = (k - 1) // 2
        kernel = np.zeros((k, k))
        if self.blur_mode == "h":
            kernel[c, :] = 1.0
        elif self.blur_mode == "v":
            kernel[:, c] = 1.0
        elif self.blur_mode == "diag_down":
            kernel = np.eye(k)
        else:
            kernel = np.flip(np.eye(k), 0)
        grid = np.repeat(np.arange(k)[:, np.newaxis], k, axis=-1)
        kernel = kernel * np.exp(-(np.square(grid - c) + np.square(grid.T - c)) / (2.0 * (k * k / 16.0)))
        kernel = kernel / np.sum(kernel)
        out = np.zeros((3, 3), dtype=np.float32)
        out[1 - c:2 + c, 1 - c:2 + c] = kernel
        return out

    def record(self):
        """(steps, kernel) as ``ops.augment_views`` takes them."""
        return self.steps(), self.blur_kernel()


def draw_augmentation() -> ViewAugmentation:
    """One ``ViewAugmentation`` from torch's and numpy's GLOBAL generators, with the reference's calls in the reference's order:
    ``ColorJitter.get_params`` (``torch.randperm(4)``, then the brightness factor, then the contrast factor, each
    ``torch.empty(1).uniform_(lo, hi)``; saturation = 0 and hue = 0 draw nothing), then ``motion_blur``'s ``np.random.choice`` of
    the mode and ``np.random.randint`` of the size.  The same ``np.random.seed`` gives the reference's mode and ksize."""
    perm = torch.randperm(4).tolist()
    b = float(torch.empty(1).uniform_(*JITTER_BRIGHTNESS))
    c = float(torch.empty(1).uniform_(*JITTER_CONTRAST))
    order = tuple(("brightness", "contrast")[i] for i in perm if i < 2)
    mode = str(np.random.choice(list(BLUR_MODES)))
    ksize = int(np.random.randint(0, (MAX_BLUR_KSIZE + 1) / 2) * 2 + 1)
    return ViewAugmentation(order=order, brightness=b, contrast=c, blur_mode=mode, ksize=ksize)


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
                 depth: torch.Tensor = None, depth_range=None, augment: Optional[ViewAugmentation] = None):
    """img_u8 uint8 [H,W,3] on the GPU (the decoded file), K [3,3] (numpy or tensor, any device) ->
    (im fp32 [3,h,w] on the GPU in [0,1], new_K fp32 [3,3] numpy, r, depth, mask).
    ``depth`` fp32 [th,tw] on the GPU with ``depth_range`` = (min_d, max_d), train mode only, gives depth fp32 [h,w] and mask bool
    [h,w] on the GPU; both are None without it.
    ``augment`` (train mode only, as the reference): the whole resized image goes through ``ops.augment_views``, which computes
    the window; None leaves the image as it is."""
    if img_u8.dim() != 3 or img_u8.shape[2] != 3:
        raise ValueError(f"prepare_view: uint8 [H,W,3] expected, got {tuple(img_u8.shape)}")
    H, W = int(img_u8.shape[0]), int(img_u8.shape[1])
    r, (rw, rh), (x0, y0, cw, ch) = view_geometry(W, H, mode, height, width, multi, resize)
    if augment is None:
        _, im = ops.resize_lanczos_u8(img_u8, (rw, rh), crop=(x0, y0, cw, ch), want_f32=True)
    else:
        if mode != "train":
            raise ValueError("prepare_view: the reference augments in train mode only")
        whole = ops.resize_lanczos_u8(img_u8, (rw, rh)) if (rw, rh) != (W, H) else img_u8
        im = ops.augment_views(whole[None], [augment], crop=(x0, y0, cw, ch))[0]
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
