#!/usr/bin/env python3
"""Generate tests/golden/colmap_array/{depth,normal}.bin with the reference's own COLMAP ``Mat`` writer
(``utils/colmap_utils.py:write_array``) for two tiny fixed arrays: a 2-D depth map [5,7] and a 3-D normal map [4,6,3].
tests/test_patch_match_cpu.py reads them back with wild_deep_mvs_amd/utils/colmap_array.py and rewrites them byte for byte.

Runs ONLY where the reference tree is available (imported the way gen_golden.py does).
Usage:  python tests/golden/gen_golden_colmap_array.py"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from gen_golden import import_reference  # noqa: E402


def arrays():
    rng = np.random.default_rng(20261016)
    depth = rng.uniform(2.0, 8.0, (5, 7)).astype(np.float32)
    depth[1, 2] = 0.0
    normal = rng.standard_normal((4, 6, 3)).astype(np.float32)
    return depth, normal


def main():
    import_reference()
    import utils.colmap_utils as cu
    out = os.path.join(HERE, "colmap_array")
    os.makedirs(out, exist_ok=True)
    depth, normal = arrays()
    cu.write_array(depth, os.path.join(out, "depth.bin"))
    cu.write_array(normal, os.path.join(out, "normal.bin"))
    print(f"wrote {out}")


if __name__ == "__main__":
    main()
