#!/usr/bin/env python3
"""Generate tests/golden/views_tiny.npz, the fixture of the image preparation: small synthetic 8-bit
images with what ``PIL.Image.resize(size, resample=Image.LANCZOS)`` returns for them, and one view with what the reference's
dataset code makes of it in train and in test mode (image, K, depth, mask).  Arrays only.

The resize cases are those of tests/test_gpu_image_prep.py, (W x H) -> (w x h): a non-integer down-scale on both axes, an
up-scale (ksize 7, bounds clipped at both edges), one axis unchanged (either one), 301 x 200 -> 5 x 7 (about 260 taps per
output), mode L, 1 x 1, and a 0 / 255 block image whose overshoot reaches both clamps.

The view: the reference's ``data/MVSDataset.py`` and ``data/md_yao.py`` are imported with ``cv2``, ``torchvision`` and ``h5py``
stood for by empty modules (here only), an ``MVSDataset`` object is made without its constructor's directory scan, and its OWN
``read_img`` (on a lossless PNG of the synthetic image), ``rescale_calib`` and ``center_crop`` are called; the three depth lines
of ``__getitem__`` (nearest ``F.interpolate`` to the image's size, the crop through ``center_crop``, the mask against the
float64 range) sit between file reads there and are written here in our words.  If the import fails the expectation comes from
PIL and the restatement; ``pv_source`` records which.

Every array written is compared with the restatement tests/_lanczos_ref.py first: a difference stops the script.
Runs ONLY where PIL (and, for the view, the reference tree) is available.  Usage:  python tests/golden/gen_golden_views.py"""
from __future__ import annotations

import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)
from gen_golden import REF  # noqa: E402  (where the reference tree lies)
from tests import _lanczos_ref as LR  # noqa: E402

# name: (W, H, channels (0 = mode L), w, h)
RESIZE_CASES = {
    "down": (53, 37, 3, 32, 32),
    "up": (47, 33, 3, 96, 64),
    "h_only": (40, 40, 3, 17, 40),
    "v_only": (40, 40, 3, 40, 17),
    "taps": (301, 200, 3, 5, 7),
    "grey": (64, 95, 0, 64, 64),
    "one": (29, 31, 3, 1, 1),
    "blocks": (70, 60, 3, 41, 37),
}
VIEW_W, VIEW_H, VIEW_HEIGHT, VIEW_WIDTH, VIEW_MULTI = 83, 61, 32, 40, 16
DEPTH_HW = (23, 31)
DEPTH_RANGE = (1.5, 6.25)                       # both exact in fp32: depths can sit ON them


def case_image(name):
    W, H, c, _, _ = RESIZE_CASES[name]
    if name == "blocks":
        return LR.block_image(H, W, c, cell=5, seed=3)
    if name == "taps":                          # large saturated areas: the accumulators come closest to the int32 range
        img = LR.block_image(H, W, c, cell=40, seed=5)
        img[::7, ::5] ^= 255
        return img
    return LR.random_image(H, W, c, seed=len(name) + W)


def view_inputs():
    rng = np.random.default_rng(11)
    img = LR.random_image(VIEW_H, VIEW_W, 3, seed=7)
    K = np.array([[520.3, 0.0, 41.7], [0.0, 522.9, 30.2], [0.0, 0.0, 1.0]], dtype=np.float32)
    depth = rng.uniform(1.0, 7.0, DEPTH_HW).astype(np.float32)
    depth[::3, ::4] = DEPTH_RANGE[0]            # on the closed end: inside
    depth[1::3, 1::4] = DEPTH_RANGE[1]          # on the open end: outside
    depth[2, 5] = np.nextafter(np.float32(DEPTH_RANGE[0]), np.float32(0))
    depth[4, 7] = np.nextafter(np.float32(DEPTH_RANGE[1]), np.float32(0))
    return img, K, depth


def reference_views(img, K, depth):
    """The two views from the reference's own methods, or None where it cannot be imported."""
    import torch
    from PIL import Image
    from torch.nn import functional as F
    sys.dont_write_bytecode = True
    for name in ("cv2", "torchvision", "torchvision.transforms", "h5py"):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    sys.modules["torchvision"].transforms = sys.modules["torchvision.transforms"]
    sys.path.insert(0, REF)
    try:
        import data.MVSDataset as base
        import data.md_yao as md
    except Exception as e:                      # noqa: BLE001
        print(f"the reference's dataset modules did not import ({type(e).__name__}: {e}): PIL + restatement")
        return None
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "view.png")
        Image.fromarray(img).save(path)
        for mode in ("train", "test"):
            ds = object.__new__(md.MVSDataset)
            base.MVSDataset.__init__(ds)
            ds.mode, ds.height, ds.width, ds.multi = mode, VIEW_HEIGHT, VIEW_WIDTH, VIEW_MULTI
            im, r = ds.read_img(path)
            new_K = ds.rescale_calib(r, K=K)
            if mode == "train":
                d = torch.tensor(depth)
                th, tw = d.shape
                d = F.interpolate(d.view(1, 1, th, tw), size=im.shape[:-1], mode="nearest").squeeze(0)
                im, new_K, d = ds.center_crop(im, K=new_K, idx=0, depth=d)
                lo, hi = np.array(DEPTH_RANGE, dtype=np.float64)
                mask = (d >= lo) & (d < hi)
                out["pv_train_depth"], out["pv_train_mask"] = d[0].numpy(), mask[0].numpy().astype(np.uint8)
            else:
                im, new_K = ds.center_crop(im, K=new_K, idx=0)
            out[f"pv_{mode}_im"] = np.ascontiguousarray(im.transpose([2, 0, 1]))
            out[f"pv_{mode}_K"], out[f"pv_{mode}_r"] = new_K, np.float64(r)
    return out


def pil_views(img, K, depth):
    from PIL import Image
    out = {}
    for mode in ("train", "test"):
        r, (rw, rh), (x0, y0, cw, ch) = LR.view_geometry(VIEW_W, VIEW_H, mode, VIEW_HEIGHT, VIEW_WIDTH, VIEW_MULTI)
        res = np.asarray(Image.fromarray(img).resize((rw, rh), resample=Image.LANCZOS)) if mode == "train" else img
        out[f"pv_{mode}_im"] = LR.to_f32_chw(res[y0:y0 + ch, x0:x0 + cw])
        out[f"pv_{mode}_K"], out[f"pv_{mode}_r"] = LR.calib(K, r, x0, y0), np.float64(r)
        if mode == "train":
            out["pv_train_depth"], out["pv_train_mask"] = LR.depth_nearest_crop(depth, (rh, rw), (y0, x0, ch, cw), *DEPTH_RANGE)
    return out


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def main():
    from PIL import Image
    import PIL
    arrays = {}
    for name, (W, H, c, w, h) in RESIZE_CASES.items():
        img = case_image(name)
        want = np.asarray(Image.fromarray(img).resize((w, h), resample=Image.LANCZOS))
        assert want.shape == ((h, w, 3) if c else (h, w)) and want.dtype == np.uint8
        assert same_bits(LR.resize(img, (w, h)), want), f"{name}: the restatement differs from PIL {PIL.__version__}"
        arrays[f"{name}_in"], arrays[f"{name}_out"] = img, want
    assert (arrays["blocks_out"] == 0).any() and (arrays["blocks_out"] == 255).any(), "the block image must reach both clamps"
    img, K, depth = view_inputs()
    views = reference_views(img, K, depth)
    source = "reference" if views is not None else "PIL + restatement"
    if views is None:
        views = pil_views(img, K, depth)
    for mode in ("train", "test"):
        im, new_K, r, d, m = LR.prepare_view(img, K, mode, VIEW_HEIGHT, VIEW_WIDTH, VIEW_MULTI, True, depth if mode == "train" else None,
                                             DEPTH_RANGE)
        assert same_bits(im, views[f"pv_{mode}_im"]), f"{mode}: image differs from the {source}"
        assert same_bits(new_K, views[f"pv_{mode}_K"]), f"{mode}: K differs from the {source}"
        assert float(r) == float(views[f"pv_{mode}_r"])
        if mode == "train":
            assert same_bits(d, views["pv_train_depth"]) and same_bits(m, views["pv_train_mask"]), f"depth / mask differ from the {source}"
            lo, hi = (np.float32(v) for v in DEPTH_RANGE)
            assert (d == lo).any() and (d == hi).any() and 0 < m.sum() < m.size, "both ends of the range must be exercised"
    arrays.update(views)
    arrays.update(pv_img=img, pv_K=K, pv_depth=depth, pv_range=np.array(DEPTH_RANGE, dtype=np.float64),
                  pv_params=np.array([VIEW_HEIGHT, VIEW_WIDTH, VIEW_MULTI], dtype=np.int64), pv_source=np.array(source))
    path = os.path.join(HERE, "views_tiny.npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB); PIL {PIL.__version__}; the view from: {source}")


if __name__ == "__main__":
    main()
