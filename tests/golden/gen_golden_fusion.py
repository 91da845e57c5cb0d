#!/usr/bin/env python3
"""Generate tests/golden/fusion_points.ply with the reference's own PLY writer (``utils/utils_ply.py:write_ply``) for fixed
arrays: float32 xyz and uint8 rgb of 10 points.  tests/test_fusion_cpu.py compares the project's writer with it byte for byte.

Runs ONLY where the reference tree is available (imported the way gen_golden.py does).
Usage:  python tests/golden/gen_golden_fusion.py"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from gen_golden import import_reference  # noqa: E402


def golden_arrays():
    """The fixed arrays of the golden file (also re-created by the test)."""
    rng = np.random.default_rng(20261016)
    xyz = (rng.standard_normal((10, 3)) * np.array([3.0, 2.0, 50.0]) + np.array([0.0, 0.0, 600.0])).astype(np.float32)
    rgb = rng.integers(0, 256, size=(10, 3), dtype=np.uint8)
    return xyz, rgb


def main():
    import_reference()
    from utils.utils_ply import write_ply
    xyz, rgb = golden_arrays()
    path = os.path.join(HERE, "fusion_points.ply")
    assert write_ply(path, [xyz, rgb], ["x", "y", "z", "red", "green", "blue"])
    print(f"wrote {path}  ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
