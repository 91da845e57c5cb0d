#!/usr/bin/env python3
"""Time ops.depth_normals (csrc/depth_normals.hip) on 49 views of 128 x 160, 49 views of 1200 x 1600 and one view of 512 x 640, each
at radius 1, 2 and 4.  Device events around a window of calls sized to last about 20 ms, after a warm-up, median of --reps
windows; one JSON line per case with
  ms_call     ops.depth_normals as a user calls it (allocates the outputs; at the small sizes this is host time),
  ms_launch   pscv_depth_normals alone into preallocated outputs (one launch per 64 views),
  hbm_floor   the least time HBM allows, 4 B read and 16 B written per pixel (normal + support) over --hbm-tbps (default 6.3, the
              measured streaming rate of the MI355X), and ms_launch as a multiple of it,
  ms_torch    a plain-torch float64 restatement of the same rule on the GPU (shifted slices, view by view): what a user would
              write without the kernel; timed once after a warm-up on one view,
and the agreement of the two (supports that differ, largest normal difference).
Usage:  python scripts/bench_depth_normals.py [--reps 7] [--cases 49x128x160,49x1200x1600,1x512x640] [--radii 1,2,4]"""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from wild_deep_mvs_amd import ops  # noqa: E402

L = ops.L
TAU, MIN_SUPPORT = 0.05, 6


def make_views(V, h, w, seed=0):
    """V depth maps of one slanted, gently curved surface with a step past the gate, 2 % holes and a masked block; pinhole K."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    ys = torch.arange(h, device="cuda", dtype=torch.float64)[:, None] / h
    xs = torch.arange(w, device="cuda", dtype=torch.float64)[None, :] / w
    rho = 0.25 + 0.03 * xs - 0.02 * ys + 0.004 * torch.sin(6.0 * xs) * torch.cos(5.0 * ys)
    depths = []
    for v in range(V):
        d = (1.0 / (rho * (1.0 + 0.01 * v))).to(torch.float32)
        d[h // 4:h // 2, w // 3:w // 2] *= 1.25
        d[torch.rand((h, w), device="cuda", generator=g) < 0.02] = 0.0
        d[h // 8:h // 8 + 5, w // 8:w // 8 + 9] = 0.0
        depths.append(d.contiguous())
    K = torch.tensor([[0.9 * w, 0.0, w / 2.0], [0.0, 0.9 * w, h / 2.0], [0.0, 0.0, 1.0]]).repeat(V, 1, 1)
    cams = ops.geo_filter_cams(K, torch.eye(3).repeat(V, 1, 1), torch.zeros(V, 3, 1)).cuda()
    return depths, cams


def torch_rule(d32, cam, r, tau, min_support):
    """The rule of INTEGRATION.md section 2n for one view in plain torch, float64 on the GPU."""
    h, w = d32.shape
    ok = (d32 > 0) & (d32 <= 3.402823466e38)
    d = torch.where(ok, d32, torch.zeros_like(d32)).double()
    rho = torch.where(ok, 1.0 / torch.where(ok, d, torch.ones_like(d)), torch.zeros_like(d))
    dP, rP = F.pad(d, (r, r, r, r)), F.pad(rho, (r, r, r, r))
    thr = tau * d
    S1, Si, Sj, Sii, Sij, Sjj, Se, Sie, Sje = (torch.zeros_like(d) for _ in range(9))
    for j in range(-r, r + 1):
        for i in range(-r, r + 1):
            dq, rq = dP[r + j:r + j + h, r + i:r + i + w], rP[r + j:r + j + h, r + i:r + i + w]
            on = ok if i == 0 and j == 0 else ok & (dq > 0) & ((dq - d).abs() <= thr)
            onf = on.double()
            e = onf * (d * rq - 1.0)
            S1 += onf
            Si += onf * i
            Sj += onf * j
            Sii += onf * (i * i)
            Sij += onf * (i * j)
            Sjj += onf * (j * j)
            Se += e
            Sie += e * i
            Sje += e * j
    C00, C01, C02 = Sjj * S1 - Sj * Sj, Sj * Si - Sij * S1, Sij * Sj - Sjj * Si
    C11, C12, C22 = Sii * S1 - Si * Si, Sij * Si - Sii * Sj, Sii * Sjj - Sij * Sij
    det = Sii * C00 + Sij * C01 + Si * C02
    A = C00 * Sie + C01 * Sje + C02 * Se
    B = C01 * Sie + C11 * Sje + C12 * Se
    g2 = det + (C02 * Sie + C12 * Sje + C22 * Se)
    fit = ok & (S1 >= min_support) & (det > 0) & (g2 > 0)
    y = torch.arange(h, device=d.device, dtype=torch.float64)[:, None].expand(h, w)
    x = torch.arange(w, device=d.device, dtype=torch.float64)[None, :].expand(h, w)
    c = cam.double()
    gc = g2 - A * x - B * y
    v = [torch.where(fit, -(c[k] * A + c[3 + k] * B + c[6 + k] * gc), -(c[9 + 3 * k] * x + c[10 + 3 * k] * y + c[11 + 3 * k]))
         for k in range(3)]
    norm = torch.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    normal = torch.stack([torch.where(ok, a / norm, torch.zeros_like(a)) for a in v], dim=-1).float()
    support = torch.where(ok, torch.where(fit, S1, -S1), torch.zeros_like(S1)).to(torch.int32)
    return normal, support


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

    inner = int(min(max(math.ceil(target_ms / max(window(1), 1e-3)), 1), 500))
    ms = [window(inner) for _ in range(reps)]
    return float(np.median(ms)), [round(x, 4) for x in ms], inner


def raw_launcher(depths, cams, r, normals, supports):
    """pscv_depth_normals into preallocated outputs: the launches alone, one per PSCV_FUSE_MAX_VIEWS views."""
    import ctypes as C
    calls = []
    for first in range(0, len(depths), L.FUSE_MAX_VIEWS):
        part = slice(first, min(first + L.FUSE_MAX_VIEWS, len(depths)))
        ptr = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
        hw = (C.c_int * (2 * len(depths[part])))(*[s for d in depths[part] for s in d.shape])
        calls.append((ptr(depths[part]), hw, part.stop - first, cams[first:].data_ptr(), ptr(normals[part]), ptr(supports[part])))

    def run():
        st = torch.cuda.current_stream().cuda_stream
        for dptr, hw, n, cptr, nptr, sptr in calls:
            L.check(L.lib().pscv_depth_normals(dptr, hw, n, cptr, r, TAU, MIN_SUPPORT, nptr, sptr, st), "pscv_depth_normals")
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cases", default="49x128x160,49x1200x1600,1x512x640")
    ap.add_argument("--radii", default="1,2,4")
    ap.add_argument("--hbm-tbps", type=float, default=6.3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_depth_normals: needs the GPU (no time is reported without one)")
    for case in a.cases.split(","):
        V, h, w = (int(x) for x in case.split("x"))
        depths, cams = make_views(V, h, w)
        pixels = V * h * w
        for r in (int(x) for x in a.radii.split(",")):
            call, call_all, inner = window_ms(lambda: ops.depth_normals(depths, cams, radius=r, rel_gate=TAU, min_support=MIN_SUPPORT,
                                                                       want_support=True), a.reps)
            normals, supports = ops.depth_normals(depths, cams, radius=r, rel_gate=TAU, min_support=MIN_SUPPORT, want_support=True)
            launch, launch_all, inner_l = window_ms(raw_launcher(depths, cams, r, normals, supports), a.reps)
            torch_rule(depths[0], cams[0], r, TAU, MIN_SUPPORT)        # warm-up of every torch kernel the restatement uses
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            bad_support, worst = 0, 0.0
            outs = []
            for v in range(V):
                outs.append(torch_rule(depths[v], cams[v], r, TAU, MIN_SUPPORT))
                if len(outs) > 1:
                    outs.pop(0)                                        # keep one view's result alive, like a streaming user would
            e1.record()
            torch.cuda.synchronize()
            ms_torch = e0.elapsed_time(e1)
            for v in range(0, V, max(V // 4, 1)):                      # agreement on a few views (outside the timed window)
                tn, ts = torch_rule(depths[v], cams[v], r, TAU, MIN_SUPPORT)
                bad_support += int((ts != supports[v]).sum())
                worst = max(worst, float((tn - normals[v]).abs().max()))
            floor_ms = pixels * 20 / (a.hbm_tbps * 1e12) * 1e3
            taps = (2 * r + 1) ** 2
            print(json.dumps({
                "case": case, "radius": r, "pixels": pixels, "ms_call": round(call, 4), "ms_call_all": call_all, "calls_per_window": inner,
                "ms_launch": round(launch, 4), "ms_launch_all": launch_all, "launches_per_window": inner_l,
                "hbm_floor_ms": round(floor_ms, 4), "launch_over_hbm_floor": round(launch / floor_ms, 2),
                "hbm_floor_fraction": round(floor_ms / launch, 3), "gpixel_per_s": round(pixels / (launch * 1e-3) / 1e9, 2),
                "gtap_per_s": round(pixels * taps / (launch * 1e-3) / 1e9, 1), "ms_torch_fp64": round(ms_torch, 2),
                "torch_over_launch": round(ms_torch / launch, 1), "supports_that_differ_from_torch": bad_support,
                "largest_normal_difference_from_torch": worst}), flush=True)


if __name__ == "__main__":
    main()
