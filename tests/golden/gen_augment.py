#!/usr/bin/env python3
"""Generate tests/golden/augment_tiny.npz, the fixture of the training-view augmentation: small
synthetic 8-bit RGB images with what PIL's OWN ``ImageEnhance.Brightness`` / ``ImageEnhance.Contrast`` return for them, so that
the GPU host needs no PIL.  Arrays only: per case ``<name>_in`` uint8 [H,W,3], ``<name>_ops`` int32 [k] (1 = brightness,
2 = contrast, in the order they run), ``<name>_factors`` float32 [k] and ``<name>_out`` uint8 [H,W,3].

The reference's function itself, ``MVSDataset.data_augmentation``, could NOT be run where this fixture was made: it needs
torchvision (``ColorJitter``) and OpenCV (``filter2D``), and neither was installed.  What is recorded is the part of it that is
PIL: torchvision's PIL path of ``ColorJitter`` calls exactly these two enhancers (stated from its source, not from a run).  The
blur has no recorded expectation; its yardstick is tests/_augment_ref.py.

The script asserts what makes the fixture bite:
  - every output equals the restatement tests/_augment_ref.py (a difference stops the script);
  - every case holds a byte where truncating the blend differs from rounding it to nearest;
  - ``clip`` (a contrast factor above 1) holds both a clipped 0 and a clipped 255;
  - ``half`` has a mean of L of exactly x.5 (PIL's int(mean + 0.5) rounds it up);
  - both orders of the two steps are present (``bc``, ``cb``).
Runs only where PIL is installed.  Usage:  python tests/golden/gen_augment.py"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
from tests import _augment_ref as AR  # noqa: E402

BRIGHTNESS, CONTRAST = 1, 2
NAMES = {BRIGHTNESS: "brightness", CONTRAST: "contrast"}
# name: (H, W, seed, [(op, factor)])
CASES = {
    "bright": (23, 31, 1, [(BRIGHTNESS, 0.8734)]),
    "bright_hi": (23, 31, 2, [(BRIGHTNESS, 1.1712)]),
    "contrast": (23, 31, 3, [(CONTRAST, 0.4219)]),
    "clip": (23, 31, 4, [(CONTRAST, 1.4537)]),
    "bc": (29, 37, 5, [(BRIGHTNESS, 1.1333), (CONTRAST, 0.7702)]),
    "cb": (29, 37, 6, [(CONTRAST, 1.3071), (BRIGHTNESS, 0.9128)]),
    "half": (8, 8, 7, [(CONTRAST, 0.6125)]),
}


def half_image(h, w, seed):
    """A grey image (R = G = B, so L is the value itself) whose mean is exactly x.5."""
    rng = np.random.default_rng(seed)
    g = rng.integers(30, 220, h * w).astype(np.int64)
    n = g.size
    assert n % 2 == 0
    diff = (int(g.sum()) // n) * n + n // 2 - int(g.sum())
    g[:abs(diff)] += 1 if diff > 0 else -1
    assert (2 * int(g.sum())) % (2 * n) == n
    return np.ascontiguousarray(np.repeat(g.reshape(h, w, 1), 3, axis=2).astype(np.uint8))


def pil_steps(img, ops, factors):
    from PIL import Image, ImageEnhance
    pil = Image.fromarray(img)
    for op, f in zip(ops, factors):
        enh = ImageEnhance.Brightness(pil) if op == BRIGHTNESS else ImageEnhance.Contrast(pil)
        pil = enh.enhance(float(f))
    return np.asarray(pil)


def main():
    import PIL
    out = {}
    for name, (h, w, seed, steps) in CASES.items():
        img = half_image(h, w, seed) if name == "half" else AR.random_image(h, w, seed)
        ops = np.array([s[0] for s in steps], dtype=np.int32)
        factors = np.array([s[1] for s in steps], dtype=np.float32)
        want = pil_steps(img, ops, factors)
        cur, bites = img, False
        for op, f in zip(ops, factors):
            deg = 0 if op == BRIGHTNESS else AR.grey_mean(cur)
            t = AR.blend_t(deg, cur, f)
            inside = (t > 0) & (t < 255)
            bites = bites or bool((inside & (np.floor(t) != np.rint(t))).any())
            if name == "clip":
                assert (t < 0).any() and (t > 255).any(), "clip: both clamps must act"
            if name == "half":
                L = AR.grey(cur).astype(np.int64)
                assert (2 * int(L.sum())) % (2 * L.size) == L.size and deg == int(L.sum()) // L.size + 1
            cur = AR.STEPS[NAMES[int(op)]](cur, f)
        assert bites, f"{name}: no byte where truncation differs from rounding"
        assert np.array_equal(cur, want), f"{name}: the restatement differs from PIL in {int((cur != want).sum())} bytes"
        if name == "clip":
            assert (want == 0).any() and (want == 255).any()
        out.update({f"{name}_in": img, f"{name}_ops": ops, f"{name}_factors": factors, f"{name}_out": want})
    assert out["bc_ops"].tolist() == [BRIGHTNESS, CONTRAST] and out["cb_ops"].tolist() == [CONTRAST, BRIGHTNESS]
    out["pil_version"] = np.array(PIL.__version__)
    path = os.path.join(HERE, "augment_tiny.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, PIL {PIL.__version__}")


if __name__ == "__main__":
    main()
