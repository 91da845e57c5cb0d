#!/usr/bin/env python3
"""Time the mesh clean-up (csrc/mesh_clean.hip; ops.mesh_components / mesh_vertex_normals / mesh_clean) on the meshes that
scripts/bench_tsdf.py extracts: 49 views of 1200 x 1600 in a grid of 640 x 512 x 256 (about 1.23 M vertices, 2.46 M faces) and
5 views of 24 x 32 in 35 x 29 x 11.  Device events around a window of calls sized to last about 20 ms, after a warm-up, median
of --reps windows; one JSON line per case with, per kernel (the launches alone, on prepared inputs),
  components   pscv_mesh_components (init, hook, flatten) and its floor at the scattered-atomic rate (--atomic-gps, default 21:
               profiles/r01_ubench_global_atomic_rate.txt): the fewest atomic operations the rule allows, one read of the parent of
               both ends of both unions of a face (4 F), one read per vertex in the flatten (V) and one swap per vertex hooked
               (at most V),
  sizes, mark, compact, normals   the other four launches and their floors over --hbm-tbps (default 6.3): the bytes each has to
               move when every gather misses (listed at `floors` below); a window repeats one call on one mesh, which stays in the
               256 MB last-level cache, so on a large mesh these kernels can come out BELOW that floor: it is a first call's,
and per ops call (torch plumbing, allocation and the host read included): mesh_components, mesh_vertex_normals,
mesh_clean(keep_largest=1, drop_degenerate=True) with and without normals.
  host         the same components and sizes with scipy.sparse.csgraph.connected_components and numpy on the host, the copy of
               the faces from the device included (timed once); labels_equal says whether its labels, mapped to the smallest
               index, equal the kernel's.
Usage:  python scripts/bench_mesh_clean.py [--reps 7] [--cases 49x1200x1600:640x512x256,5x24x32:35x29x11]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_tsdf import TRUNC_VOXELS, make_views, window_ms  # noqa: E402
from wild_deep_mvs_amd import ops  # noqa: E402

L = ops.L


def extract_mesh(V, h, w, dims):
    depths, colors, cams = make_views(V, h, w)
    voxel = 6.4 / dims[0]
    origin = (-0.5 * voxel * (dims[0] - 1), -0.5 * voxel * (dims[1] - 1), 4.0 - 0.5 * voxel * (dims[2] - 1))
    state = ops.tsdf_volume(dims)
    ops.tsdf_integrate(state, depths, [ops.pack_rgba8(c) for c in colors], cams, origin=origin, voxel=voxel, trunc=TRUNC_VOXELS * voxel)
    return ops.tsdf_extract(state, origin=origin, voxel=voxel, min_weight=1)


def host_components(faces, n):
    """(label, fcount, vcount, seconds): scipy + numpy on the host, the copy from the device included."""
    import scipy.sparse as sparse
    from scipy.sparse.csgraph import connected_components
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f = faces.cpu().numpy().astype(np.int64)
    rows, cols = np.concatenate((f[:, 0], f[:, 0])), np.concatenate((f[:, 1], f[:, 2]))
    graph = sparse.coo_matrix((np.ones(rows.size, dtype=np.int8), (rows, cols)), shape=(n, n))
    _, comp = connected_components(graph, directed=False)
    smallest = np.full(comp.max() + 1, n, dtype=np.int64)
    np.minimum.at(smallest, comp, np.arange(n))
    label = smallest[comp].astype(np.int32)
    fcount = np.bincount(label[f[:, 0]], minlength=n).astype(np.int32)
    vcount = np.bincount(label, minlength=n).astype(np.int32)
    return label, fcount, vcount, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cases", default="49x1200x1600:640x512x256,5x24x32:35x29x11")
    ap.add_argument("--hbm-tbps", type=float, default=6.3)
    ap.add_argument("--atomic-gps", type=float, default=21.0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_clean: needs the GPU (no time is reported without one)")
    lib = L.lib()
    stream = lambda: torch.cuda.current_stream().cuda_stream
    for case in a.cases.split(","):
        views, grid = case.split(":")
        V, h, w = (int(x) for x in views.split("x"))
        xyz, rgb, faces = extract_mesh(V, h, w, tuple(int(x) for x in grid.split("x")))
        torch.cuda.empty_cache()
        nv, nf = int(xyz.shape[0]), int(faces.shape[0])
        i32 = lambda n, fill=None: (torch.empty(n, dtype=torch.int32, device="cuda") if fill is None else
                                    torch.full((n,), fill, dtype=torch.int32, device="cuda"))
        label, status, fcount, vcount = i32(nv), i32(2, 0), i32(nv, 0), i32(nv, 0)

        def components():
            L.check(lib.pscv_mesh_components(faces.data_ptr(), nf, nv, label.data_ptr(), status.data_ptr(), stream()), "components")
        k_comp, k_comp_all, inner = window_ms(components, a.reps)

        def sizes():                                                   # (the counts keep growing over the window: timing only)
            L.check(lib.pscv_mesh_component_sizes(label.data_ptr(), faces.data_ptr(), nf, nv, fcount.data_ptr(), vcount.data_ptr(), stream()), "sizes")
        k_sizes, _, _ = window_ms(sizes, a.reps)
        got = ops.mesh_components(faces, nv)
        h_label, h_fcount, h_vcount, host_s = host_components(faces, nv)
        equal = bool((got[0].cpu().numpy() == h_label).all() and (got[1].cpu().numpy() == h_fcount).all() and (got[2].cpu().numpy() == h_vcount).all())
        fc = got[1]
        keep_comp = (fc == fc.max()).to(torch.uint8)
        fmark, vmark = i32(nf), i32(nv, 0)

        def mark():
            L.check(lib.pscv_mesh_mark(xyz.data_ptr(), faces.data_ptr(), got[0].data_ptr(), keep_comp.data_ptr(), nf, nv, 1, fmark.data_ptr(),
                                       vmark.data_ptr(), stream()), "mark")
        k_mark, _, _ = window_ms(mark, a.reps)
        fincl, vincl = torch.cumsum(fmark, 0, dtype=torch.int32), torch.cumsum(vmark, 0, dtype=torch.int32)
        nf2, nv2 = int(fincl[-1]), int(vincl[-1])
        normals = ops.mesh_vertex_normals(xyz, faces)
        o_xyz, o_rgb, o_nrm, o_faces = torch.empty_like(xyz[:nv2]), torch.empty_like(rgb[:nv2]), torch.empty_like(xyz[:nv2]), torch.empty_like(faces[:nf2])

        def compact():
            L.check(lib.pscv_mesh_compact(xyz.data_ptr(), rgb.data_ptr(), normals.data_ptr(), faces.data_ptr(), fmark.data_ptr(), vmark.data_ptr(),
                                          fincl.data_ptr(), vincl.data_ptr(), nf, nv, o_xyz.data_ptr(), o_rgb.data_ptr(), o_nrm.data_ptr(),
                                          o_faces.data_ptr(), nf2, nv2, stream()), "compact")
        k_compact, _, _ = window_ms(compact, a.reps)
        key = faces.reshape(-1).to(torch.int64)
        corners = torch.sort(key, stable=True).indices.to(torch.int32)
        corner_off = torch.zeros(nv + 1, dtype=torch.int32, device="cuda")
        corner_off[1:] = torch.cumsum(torch.bincount(key, minlength=nv), 0)

        def vnormals():
            L.check(lib.pscv_mesh_vertex_normals(xyz.data_ptr(), faces.data_ptr(), corner_off.data_ptr(), corners.data_ptr(), nf, nv,
                                                 normals.data_ptr(), stream()), "normals")
        k_normals, _, _ = window_ms(vnormals, a.reps)
        o_comp, o_comp_all, _ = window_ms(lambda: ops.mesh_components(faces, nv), a.reps)
        o_nrm_ms, _, _ = window_ms(lambda: ops.mesh_vertex_normals(xyz, faces), a.reps)
        o_clean, o_clean_all, _ = window_ms(lambda: ops.mesh_clean(xyz, rgb, faces, keep_largest=1, drop_degenerate=True), a.reps)
        o_clean_n, _, _ = window_ms(lambda: ops.mesh_clean(xyz, rgb, faces, keep_largest=1, drop_degenerate=True, normals=normals), a.reps)
        hbm = lambda nbytes: nbytes / (a.hbm_tbps * 1e12) * 1e3
        floors = {"components_atomic": (4 * nf + 2 * nv) / (a.atomic_gps * 1e9) * 1e3,
                  "sizes": hbm(12 * nf + 4 * nf + 4 * nv),                                  # faces, label[first vertex], label
                  "mark": hbm(12 * nf + 4 * nf + nf + 36 * nf + 4 * nf + 12 * nf),          # + keep_comp, three positions, fmark, vmark stores
                  "compact": hbm(8 * (nf + nv) + 12 * nf + 12 * nf + 27 * nv + 12 * nf2 + 27 * nv2),
                  "normals": hbm(3 * nf * (4 + 12 + 36) + 8 * nv + 12 * nv)}                # per corner: its id, the face, three positions
        times = {"components_atomic": k_comp, "sizes": k_sizes, "mark": k_mark, "compact": k_compact, "normals": k_normals}
        print(json.dumps({
            "case": case, "vertices": nv, "faces": nf, "components_with_faces": int((fc > 0).sum()), "largest_component_faces": int(fc.max()),
            "kept_faces": nf2, "kept_vertices": nv2,
            "kernel_ms": {"components": round(k_comp, 4), "components_all": k_comp_all, "launches_per_window": inner, "sizes": round(k_sizes, 4),
                          "mark": round(k_mark, 4), "compact": round(k_compact, 4), "normals": round(k_normals, 4)},
            "floor_ms": {k: round(v, 5) for k, v in floors.items()},
            "over_floor": {k: round(times[k] / v, 2) for k, v in floors.items()},
            "ops_ms": {"mesh_components": round(o_comp, 4), "mesh_components_all": o_comp_all, "mesh_vertex_normals": round(o_nrm_ms, 4),
                       "mesh_clean": round(o_clean, 4), "mesh_clean_all": o_clean_all, "mesh_clean_with_normals": round(o_clean_n, 4)},
            "host": {"scipy_numpy_ms": round(host_s * 1e3, 2), "over_ops_mesh_components": round(host_s * 1e3 / o_comp, 1), "labels_equal": equal},
            "status_words": status.tolist()}), flush=True)
        del xyz, rgb, faces
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
