#!/usr/bin/env python3
"""Time ops.tsdf_integrate and ops.tsdf_extract (csrc/tsdf_fusion.hip) on 49 views of 1200 x 1600 into a DTU-like grid of
640 x 512 x 256 (voxel 0.01 at depth 4, about 3.6 pixel footprints) and on 5 views of 24 x 32 into 35 x 29 x 11.  Device events around a window of calls sized to last about 20 ms,
after a warm-up, median of --reps windows; one JSON line per case with
  integrate.ms_call     ops.tsdf_integrate as a user calls it (packs the colours, takes each view's largest depth with torch),
  integrate.ms_launch   pscv_tsdf_integrate alone on prepared inputs,
  integrate.ms_culled   the same launch with the grid moved outside every frustum: what a tile costs when no view touches it,
  integrate.hbm_floor   the least time HBM allows for the state traffic, 24 B read and 24 B written per voxel over --hbm-tbps
                        (default 6.3, the measured streaming rate of the MI355X), and ms_launch as a multiple of it,
  integrate.ms_torch    a plain-torch float64 restatement of the same rule on the GPU (all voxels at once, view by view): what a
                        user would write without the kernel; timed once after a warm-up on one view; and the entries of the
                        state that differ between the two,
  extract.ms_call       ops.tsdf_extract (mark, two prefix sums and one host read with torch, two emits; allocates its outputs),
  extract.ms_mark / ms_emit   the three launches alone on prepared prefix sums,
  extract.hbm_floor     32 B per voxel (mark: 8 read, 4 written; the emits read the mark and their prefix sums: 8 and 12).
Usage:  python scripts/bench_tsdf.py [--reps 7] [--cases 49x1200x1600:640x512x256,5x24x32:35x29x11]"""
import argparse
import ctypes as C
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from wild_deep_mvs_amd import ops  # noqa: E402

L = ops.L
TRUNC_VOXELS = 3.0


def make_views(V, h, w, seed=0):
    """V pinhole cameras on a square grid in the plane z = 0 looking along +z at the plane n . X = c0 near z = 4 (the layout of
    synthetic.make_fusion_scene without the tilt), built on the GPU: analytic depths with 1 % holes, random colours."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    n = torch.tensor([0.10, -0.06, 1.0], dtype=torch.float64)
    n = n / n.norm()
    c0 = 4.0 * float(n[2])
    side = int(math.ceil(math.sqrt(V)))
    f = 0.9 * w
    K = torch.tensor([[f, 0.0, w / 2.0], [0.0, f, h / 2.0], [0.0, 0.0, 1.0]], dtype=torch.float64)
    ys = torch.arange(h, device="cuda", dtype=torch.float64)[:, None].expand(h, w)
    xs = torch.arange(w, device="cuda", dtype=torch.float64)[None, :].expand(h, w)
    ray = torch.stack(((xs - w / 2.0) / f, (ys - h / 2.0) / f, torch.ones_like(xs)), dim=-1)
    depths, colors, ts = [], [], []
    for v in range(V):
        c = torch.tensor([(v % side - (side - 1) / 2.0) * 0.25, (v // side - (side - 1) / 2.0) * 0.25, 0.0], dtype=torch.float64)
        d = ((c0 - float(n @ c)) / (ray @ n.cuda())).to(torch.float32)
        d[torch.rand((h, w), device="cuda", generator=g) < 0.01] = 0.0
        depths.append(d.contiguous())
        colors.append(torch.randint(0, 256, (h, w, 3), device="cuda", generator=g, dtype=torch.uint8))
        ts.append(-c.reshape(3, 1))
    cams = ops.geo_filter_cams(K.repeat(V, 1, 1), torch.eye(3).repeat(V, 1, 1), torch.stack(ts)).cuda()
    return depths, colors, cams


def torch_integrate_view(S, W, RGB, CW, X, Y, Z, d32, col, cam, trunc):
    """One view of the rule of INTEGRATION.md section 2o in plain torch, float64 on the GPU; the state tensors are fp64 / int64."""
    c = cam.double()
    K, R, t = c[0:9], c[18:27], c[27:30]
    e = [R[3 * r] * X + R[3 * r + 1] * Y + R[3 * r + 2] * Z + t[r] for r in range(3)]
    x, y, z = (K[3 * r] * e[0] + K[3 * r + 1] * e[1] + K[3 * r + 2] * e[2] for r in range(3))
    h, w = d32.shape
    px, py = torch.floor(x / z + 0.5), torch.floor(y / z + 0.5)
    on = (z > 0) & (px >= 0) & (px < w) & (py >= 0) & (py < h)
    o = torch.where(on, py * w + px, torch.zeros_like(px)).long()
    d = d32.reshape(-1)[o]
    on &= (d > 0) & (d <= 3.402823466e38)
    sd = d.double() - z
    on &= ~(sd < -trunc)
    q = sd / torch.full((), trunc, dtype=torch.float64, device=sd.device)    # (a device tensor: torch divides by a host scalar as a
                                                                             # product with its reciprocal, which rounds differently)
    S += torch.where(on, torch.where(q < 1.0, q, torch.ones_like(q)), torch.zeros_like(q))
    W += on
    near = on & (sd <= trunc)
    RGB += torch.where(near[..., None], col.reshape(-1, 3)[o].long(), torch.zeros((), dtype=torch.long, device=S.device))
    CW += near


def window_ms(fn, reps, target_ms=20.0):
    """Median over `reps` windows of the time per call; a window holds enough calls to last about target_ms."""
    fn()                                                              # warm-up
    torch.cuda.synchronize()

    def window(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    inner = int(min(max(math.ceil(target_ms / max(window(1), 1e-3)), 1), 200))
    ms = [window(inner) for _ in range(reps)]
    return float(np.median(ms)), [round(x, 4) for x in ms], inner


def raw_integrate(state, depths, packed, cams, origin, voxel, trunc):
    """pscv_tsdf_integrate on prepared inputs: the launches alone, one per PSCV_FUSE_MAX_VIEWS views."""
    nx, ny, nz = state.dims
    calls, keep = [], []
    for first in range(0, len(depths), L.FUSE_MAX_VIEWS):
        part = slice(first, min(first + L.FUSE_MAX_VIEWS, len(depths)))
        ptr = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
        hw = (C.c_int * (2 * len(depths[part])))(*[s for d in depths[part] for s in d.shape])
        dmax = ops._max_valid_depth(depths[part])
        keep.append(dmax)
        calls.append((ptr(depths[part]), ptr(packed[part]), hw, part.stop - first, cams[first:].data_ptr(), dmax.data_ptr()))

    def run():
        st = torch.cuda.current_stream().cuda_stream
        for dptr, cptr, hw, n, camptr, mptr in calls:
            L.check(L.lib().pscv_tsdf_integrate(dptr, cptr, hw, n, camptr, mptr, origin[0], origin[1], origin[2], voxel, trunc, nx, ny, nz,
                                                state.tsdf_sum.data_ptr(), state.weight.data_ptr(), state.rgb_sum.data_ptr(),
                                                state.cweight.data_ptr(), st), "pscv_tsdf_integrate")
    run.keep = keep
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cases", default="49x1200x1600:640x512x256,5x24x32:35x29x11")
    ap.add_argument("--hbm-tbps", type=float, default=6.3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tsdf: needs the GPU (no time is reported without one)")
    for case in a.cases.split(","):
        views, grid = case.split(":")
        V, h, w = (int(x) for x in views.split("x"))
        dims = tuple(int(x) for x in grid.split("x"))
        nvox = dims[0] * dims[1] * dims[2]
        depths, colors, cams = make_views(V, h, w)
        packed = [ops.pack_rgba8(c) for c in colors]
        # the grid: 6.4 wide, centred on the plane in front of the rig (the views cover about 5.5 x 4.2 of it at depth 4)
        voxel = 6.4 / dims[0]
        origin = (-0.5 * voxel * (dims[0] - 1), -0.5 * voxel * (dims[1] - 1), 4.0 - 0.5 * voxel * (dims[2] - 1))
        trunc = TRUNC_VOXELS * voxel
        kw = dict(origin=origin, voxel=voxel, trunc=trunc)

        state = ops.tsdf_volume(dims)

        def call():
            state.views = 0                                           # (timing only: the view limit guards real colour sums)
            ops.tsdf_integrate(state, depths, packed, cams, **kw)
        i_call, i_call_all, inner = window_ms(call, a.reps)
        i_launch, i_launch_all, inner_l = window_ms(raw_integrate(state, depths, packed, cams, origin, voxel, trunc), a.reps)
        away = (origin[0] + 1000.0, origin[1], origin[2])
        i_culled, _, _ = window_ms(raw_integrate(state, depths, packed, cams, away, voxel, trunc), a.reps)

        # one clean integration for the comparison and for the extraction
        state = ops.tsdf_volume(dims)
        ops.tsdf_integrate(state, depths, packed, cams, **kw)
        nx, ny, nz = dims
        kk, jj, ii = torch.meshgrid(torch.arange(nz, device="cuda", dtype=torch.float64), torch.arange(ny, device="cuda", dtype=torch.float64),
                                    torch.arange(nx, device="cuda", dtype=torch.float64), indexing="ij")
        X, Y, Z = origin[0] + ii * voxel, origin[1] + jj * voxel, origin[2] + kk * voxel
        del kk, jj, ii
        fresh = lambda: (torch.zeros((nz, ny, nx), dtype=torch.float64, device="cuda"), torch.zeros((nz, ny, nx), dtype=torch.long, device="cuda"),
                         torch.zeros((nz, ny, nx, 3), dtype=torch.long, device="cuda"), torch.zeros((nz, ny, nx), dtype=torch.long, device="cuda"))
        torch_integrate_view(*fresh(), X, Y, Z, depths[0], colors[0], cams[0], trunc)     # warm-up of every torch kernel used
        S, Wt, RGB, CW = fresh()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for v in range(V):
            torch_integrate_view(S, Wt, RGB, CW, X, Y, Z, depths[v], colors[v], cams[v], trunc)
        e1.record()
        torch.cuda.synchronize()
        ms_torch = e0.elapsed_time(e1)
        differ = int((S.float() != state.tsdf_sum).sum()) + int((Wt != state.weight).sum()) + int((RGB.float() != state.rgb_sum).sum()) + \
            int((CW != state.cweight).sum())
        observed = int((Wt > 0).sum())
        del S, Wt, RGB, CW, X, Y, Z

        ekw = dict(origin=origin, voxel=voxel, min_weight=1)
        x_call, x_call_all, inner_x = window_ms(lambda: ops.tsdf_extract(state, **ekw), a.reps)
        xyz, rgb, faces = ops.tsdf_extract(state, **ekw)
        info = torch.empty(nvox, dtype=torch.int32, device="cuda")
        lib = L.lib()
        stream = lambda: torch.cuda.current_stream().cuda_stream
        mark = lambda: L.check(lib.pscv_tsdf_mark(state.tsdf_sum.data_ptr(), state.weight.data_ptr(), nx, ny, nz, 1, info.data_ptr(), stream()),
                               "pscv_tsdf_mark")
        x_mark, _, _ = window_ms(mark, a.reps)
        counts = info.view(torch.uint8).view(nvox, 4)[:, 2:]
        vincl = torch.cumsum(counts[:, 0], dim=0, dtype=torch.int32)
        fincl = torch.cumsum(counts[:, 1], dim=0, dtype=torch.int32)

        def emit():
            L.check(lib.pscv_tsdf_emit_vertices(state.tsdf_sum.data_ptr(), state.weight.data_ptr(), state.rgb_sum.data_ptr(),
                                                state.cweight.data_ptr(), info.data_ptr(), vincl.data_ptr(), nx, ny, nz, origin[0], origin[1],
                                                origin[2], voxel, xyz.data_ptr(), rgb.data_ptr(), xyz.shape[0], stream()), "emit_vertices")
            L.check(lib.pscv_tsdf_emit_faces(info.data_ptr(), vincl.data_ptr(), fincl.data_ptr(), nx, ny, nz, faces.data_ptr(), faces.shape[0],
                                             stream()), "emit_faces")
        x_emit, _, _ = window_ms(emit, a.reps) if xyz.shape[0] else (0.0, None, None)
        i_floor = nvox * 48 / (a.hbm_tbps * 1e12) * 1e3
        x_floor = nvox * 32 / (a.hbm_tbps * 1e12) * 1e3
        print(json.dumps({
            "case": case, "voxels": nvox, "voxel": round(voxel, 5), "observed_voxels": observed,
            "integrate": {"ms_call": round(i_call, 4), "ms_call_all": i_call_all, "calls_per_window": inner, "ms_launch": round(i_launch, 4),
                          "ms_launch_all": i_launch_all, "launches_per_window": inner_l, "ms_culled": round(i_culled, 4),
                          "hbm_floor_ms": round(i_floor, 4), "launch_over_hbm_floor": round(i_launch / i_floor, 2),
                          "gvoxel_view_per_s": round(nvox * V / (i_launch * 1e-3) / 1e9, 1), "ms_torch_fp64": round(ms_torch, 2),
                          "torch_over_launch": round(ms_torch / i_launch, 1), "state_entries_that_differ_from_torch": differ},
            "extract": {"vertices": int(xyz.shape[0]), "faces": int(faces.shape[0]), "ms_call": round(x_call, 4), "ms_call_all": x_call_all,
                        "calls_per_window": inner_x, "ms_mark": round(x_mark, 4), "ms_emit": round(x_emit, 4),
                        "hbm_floor_ms": round(x_floor, 4), "launches_over_hbm_floor": round((x_mark + x_emit) / x_floor, 2)}}), flush=True)
        del state, info, depths, colors, packed
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
