"""CPU: the argument checks shared by the multi-view geometry operators (fuse_depth_*, colmap_fuse*, view_covisibility,
depth_normals, point_world_normals, tsdf_integrate, tsdf_brick_probe, tsdf_brick_integrate), as a record of their behaviour.

The C entry points are called with fake non-null addresses and exactly one bad argument each: every call is refused before a
launch (rc == -1) and the whole text of pscv_last_error() is compared.  The Python operators are called with exactly one rule
broken and must raise the recorded exception type with the operator's prefix and the phrase that names the rule.  The expected texts were written down from the
library before the view table, the TSDF call set-up and the ops.py input checks were shared, and did not change with that."""
import ctypes as C

import pytest
import torch

from wild_deep_mvs_amd import _lib as L, ops

VP = C.c_void_p
A = 64                                                    # a non-null address; no call below gets far enough to use it


def ptrs(n, null_at=None):
    return (VP * n)(*[None if v == null_at else A for v in range(n)])


def sizes(n, change=None):
    """(h, w) = (5, 7) for n views; change = {view: (h, w)}"""
    flat = []
    for v in range(n):
        flat += list((change or {}).get(v, (5, 7)))
    return (C.c_int * (2 * n))(*flat)


# ---- one row per entry point: the valid argument list for n views (built by `args`), the positions of n_views, hw, the depth
# array and the companion arrays, the lower bound of n_views, and a change that makes a call with good views fail afterwards ----
def fuse_args(n):
    return [0, ptrs(n), ptrs(n), ptrs(n), sizes(n), n, A, 0.01, 3, 1e-3, 1e5, A, A, A, A, 100, A, A, 1 << 40]


def colmap_args(n):
    return [0, 0, ptrs(n), ptrs(n), ptrs(n), ptrs(n), sizes(n), n, A, (C.c_long * n)(), 0, 0.01, 1.0, 3, 100, A, A, A, A, A, 100, A, A,
            1 << 40]


def colmap_normals_args(n):
    a = colmap_args(n)
    return a[:15] + [ptrs(n), 10.0] + a[15:]


def covis_args(n):
    return [ptrs(n), sizes(n), n, A, 1, 0.01, A, A, 1 << 40]


def normals_args(n):
    return [ptrs(n), sizes(n), n, A, 2, 0.05, 6, ptrs(n), ptrs(n)]


def pwn_args(n):
    return [A, A, 1, ptrs(n), sizes(n), n, A, A]


def tsdf_args(n):
    return [ptrs(n), ptrs(n), sizes(n), n, A, A, 0.0, 0.0, 0.0, 0.5, 1.5, 4, 3, 2, A, A, A, A]


def probe_args(n):
    return [ptrs(n), sizes(n), n, A, A, A, 0.0, 0.0, 0.0, 0.5, 1.5, 9, 8, 7, A]


def brick_args(n):
    return [ptrs(n), ptrs(n), sizes(n), n, A, A, 0.0, 0.0, 0.0, 0.5, 1.5, 9, 8, 7, A, 2, A, A, A, A]


# name: (args, index of n_views, of hw, of depth (None: the entry point takes none), {companion index: message tail}, lower bound,
#        upper bound (None: none), (change, message) of the call that fails after a 46340 x 46340 view 0 passed)
NULL = "view 1 has a null pointer"
ENTRY = {
    "pscv_fuse_depth_pass": (fuse_args, 5, 4, 1, {2: NULL, 3: NULL}, 2, 64, ({18: 0}, "workspace of 0 bytes < 35184850176")),
    "pscv_colmap_fuse_pass": (colmap_args, 7, 6, 2, {3: NULL, 4: NULL, 5: NULL}, 2, 64,
                              ({23: 0}, "workspace of 0 bytes < 71266692096")),
    "pscv_colmap_fuse_pass_normals": (colmap_normals_args, 7, 6, 2, {3: NULL, 4: NULL, 5: NULL, 15: "view 1 has a null normal map"}, 2,
                                      64, ({25: 0}, "workspace of 0 bytes < 71266692096")),
    "pscv_view_covisibility": (covis_args, 2, 1, 0, {}, 2, None,
                               ({}, "2147395600 samples in one view: more than 65535 tiles of 256 (raise the stride)")),
    "pscv_depth_normals": (normals_args, 2, 1, 0, {7: NULL, 8: NULL}, 1, 64, ({7: ptrs(3, 1)}, NULL)),
    "pscv_point_world_normals": (pwn_args, 5, 4, None, {3: NULL}, 1, 64, ({0: None}, "null pointer argument")),
    "pscv_tsdf_integrate": (tsdf_args, 3, 2, 0, {1: NULL}, 1, 64, ({1: ptrs(3, 1)}, NULL)),
    "pscv_tsdf_brick_probe": (probe_args, 2, 1, 0, {}, 1, 64, ({1: sizes(3, {0: (46340, 46340), 1: (0, 7)})}, "view 1 has bad size 0x7")),
    "pscv_tsdf_brick_integrate": (brick_args, 3, 2, 0, {1: NULL}, 1, 64, ({16: None}, "null pointer argument")),
}


def refused(name, args, change):
    lib = L.lib()
    args = list(args)
    for k, v in change.items():
        args[k] = v
    assert getattr(lib, name)(*args, None) == -1, (name, change)
    return lib.pscv_last_error().decode()


@pytest.mark.parametrize("name", list(ENTRY))
def test_c_entry_point_refuses_one_bad_view_argument(name):
    make, i_n, i_hw, i_depth, companions, lo, hi, (late_change, late_text) = ENTRY[name]
    ok = make(3)
    # the view count: one below the lower bound and, where there is an upper bound, one above it
    if hi is None:
        assert refused(name, ok, {i_n: lo - 1}) == f"{name}: n_views={lo - 1} < {lo}"
    else:
        assert refused(name, ok, {i_n: lo - 1}) == f"{name}: n_views={lo - 1} outside [{lo},{hi}]"
        assert refused(name, ok, {i_n: hi + 1}) == f"{name}: n_views={hi + 1} outside [{lo},{hi}]"
    # a null depth pointer at the last view, a null in each companion array at view 1
    if i_depth is not None:
        assert refused(name, ok, {i_depth: ptrs(3, 2)}) == f"{name}: view 2 has a null pointer"
    for k, text in companions.items():
        assert refused(name, ok, {k: ptrs(3, 1)}) == f"{name}: {text}"
    # sizes: a zero or negative side, and h w = 2^31
    for h, w in ((0, 7), (5, 0), (-1, 7), (65536, 32768)):
        assert refused(name, ok, {i_hw: sizes(3, {1: (h, w)})}) == f"{name}: view 1 has bad size {h}x{w}"
    # 46340 x 46340 < 2^31 passes the size check: the call fails on the later argument chosen to be bad
    change = {i_hw: sizes(3, {0: (46340, 46340)})}
    change.update(late_change)
    assert refused(name, ok, change) == f"{name}: {late_text}"


# ---- the Python operators: exactly one rule broken ---------------------------------------------------------------------------------
def views(n=2, device="cpu"):
    depths = [torch.ones(5, 7, device=device) for _ in range(n)]
    colors = [torch.zeros(5, 7, 3, dtype=torch.uint8, device=device) for _ in range(n)]
    eye = torch.eye(3)[None].repeat(n, 1, 1)
    return depths, colors, ops.geo_filter_cams(eye, eye, torch.zeros(n, 3, 1)).to(device)


GRID = dict(origin=(0.0, 0.0, 0.0), voxel=0.5, trunc=1.5)


def brick_volume(device="cpu"):
    return ops.tsdf_bricks(torch.zeros((1, 1, 2), dtype=torch.int32, device=device), (9, 8, 7))


# operator: (call(depths, colors, cams, device), the prefix of its messages, takes colours, casts its depth maps to fp32)
OPERATORS = {
    "fuse_depth_maps": (lambda d, c, cams, dev: ops.fuse_depth_maps(d, c, cams), "pscv.fuse_depth", True, True),
    "fuse_depth_pass": (lambda d, c, cams, dev: ops.fuse_depth_pass(0, d, c, cams, [torch.zeros(5, 7, dtype=torch.uint8, device=dev)] * 2),
                        "pscv.fuse_depth", True, True),
    "colmap_fuse": (lambda d, c, cams, dev: ops.colmap_fuse(d, c, cams, [[1], [0]], max_depth_error=0.01, max_reproj_error=1.0,
                                                            min_num_pixels=2), "pscv.fuse_depth", True, True),
    "colmap_fuse_pass": (lambda d, c, cams, dev: ops.colmap_fuse_pass(0, d, c, cams, [[1], [0]],
                                                                      [torch.zeros(5, 7, dtype=torch.uint8, device=dev)] * 2),
                         "pscv.fuse_depth", True, True),
    "view_covisibility": (lambda d, c, cams, dev: ops.view_covisibility(d, cams, max_depth_error=0.01), "pscv.view_covisibility", False, True),
    "depth_normals": (lambda d, c, cams, dev: ops.depth_normals(d, cams), "pscv.depth_normals", False, True),
    "tsdf_integrate": (lambda d, c, cams, dev: ops.tsdf_integrate(ops.tsdf_volume((4, 3, 2), dev), d, c, cams, **GRID),
                       "pscv.tsdf_integrate", True, False),
    "tsdf_brick_probe": (lambda d, c, cams, dev: ops.tsdf_brick_probe(d, cams, (9, 8, 7), **GRID), "pscv.tsdf_brick_probe", False, False),
    "tsdf_brick_integrate": (lambda d, c, cams, dev: ops.tsdf_brick_integrate(brick_volume(dev), d, c, cams, **GRID),
                             "pscv.tsdf_brick_integrate", True, False),
}


FP32_MAP, CAMS, COLOURS = r"fp32 \[h,w\]", "cams", "colours of view 1"


def one_violation_cases(device, colours, casts):
    """(a phrase of the message that names the broken rule, depths, colors, cams) for the rules every operator of the family shares"""
    d, c, cams = views(2, device)
    out = [(FP32_MAP, [d[0], torch.ones(5, 7, 1, device=device)], c, cams),               # a 3-D depth map
           (CAMS, d, c, cams[:, :29].contiguous()),                                       # cams [V,29]
           (CAMS, d, c, cams[:1]),                                                        # cams with V - 1 rows
           (CAMS, d, c, torch.cat((cams, cams[:1])))]                                     # cams with V + 1 rows
    if not casts:
        out.append((FP32_MAP, [d[0], d[1].double()], c, cams))                            # a depth map that is not fp32
    if colours:
        out.append((COLOURS, d, [c[0], torch.zeros(5, 6, 3, dtype=torch.uint8, device=device)], cams))   # a colour image of another size
    return out


def world_normals(normals, cams, device):
    idx = torch.zeros(1, dtype=torch.int32, device=device)
    return ops.point_world_normals(idx, idx, normals, cams)


@pytest.mark.parametrize("name", list(OPERATORS))
def test_operator_has_no_cpu_path(name):
    call, prefix, colours, casts = OPERATORS[name]
    with pytest.raises(RuntimeError, match="no CPU"):
        call(*views(2), "cpu")


def test_point_world_normals_has_no_cpu_path():
    with pytest.raises(RuntimeError, match="no CPU"):
        world_normals([torch.zeros(5, 7, 3)] * 2, views(2)[2], "cpu")


@pytest.mark.parametrize("name", [k for k, v in OPERATORS.items() if not v[3]])
def test_tsdf_operator_names_one_bad_argument_without_a_gpu(name):
    """The operators that do not cast check their arguments before they look at the device."""
    call, prefix, colours, casts = OPERATORS[name]
    for phrase, d, c, cams in one_violation_cases("cpu", colours, casts):
        with pytest.raises(ValueError, match=f"^{prefix}: .*{phrase}"):
            call(d, c, cams, "cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(OPERATORS))
def test_operator_names_one_bad_argument(name):
    call, prefix, colours, casts = OPERATORS[name]
    for phrase, d, c, cams in one_violation_cases("cuda", colours, casts):
        with pytest.raises(ValueError, match=f"^{prefix}: .*{phrase}"):
            call(d, c, cams, "cuda")
    d, c, cams = views(2, "cuda")
    with pytest.raises(RuntimeError, match="no CPU"):                       # one CPU tensor among valid arguments
        call([d[0], d[1].cpu()], c, cams, "cuda")


@pytest.mark.gpu
def test_point_world_normals_names_one_bad_argument():
    normals, cams = [torch.zeros(5, 7, 3, device="cuda")] * 2, views(2, "cuda")[2]
    for bad in (cams[:, :29].contiguous(), cams[:1], torch.cat((cams, cams[:1]))):
        with pytest.raises(ValueError, match="^pscv.point_world_normals: .*cams"):
            world_normals(normals, bad, "cuda")
    with pytest.raises(ValueError, match="^pscv.point_world_normals: normal map 1"):
        world_normals([normals[0], torch.zeros(5, 7, device="cuda")], cams, "cuda")
    with pytest.raises(RuntimeError, match="no CPU"):
        world_normals([normals[0], normals[1].cpu()], cams, "cuda")
    assert world_normals(normals, cams, "cuda").shape == (1, 3)
